// Coarse, host-language-neutral entry points: pk_ctx_* / pk_mat_* / pk_svd_build / pk_score_topk.
//
// Everything above the kernels that polara_amd's Python layer does with torch tensors — the block Chebyshev-filtered
// eigensolver of `SVDModel.build` (models.py:835-855 -> svds) and the recommendation pass of `get_recommendations`
// (models.py:391-405, 857-861, 494-519, 488-491) — restated in C++ on top of the same kernel launchers, with
// caller-allocated HOST outputs, device memory owned by the library behind opaque handles, and one mutex per context
// so that the reference's thread-pool pattern (models.py:374-382) is safe.  A host in any language binds five
// functions and needs neither Python nor torch (tests/test_coarse_abi.py drives them through ctypes alone).
//
// The algorithms are those of polara_amd/solver.py and polara_amd/scoring.py, function by function; only the memory
// management differs (a per-context pool of hipMalloc'd blocks instead of torch tensors) and the start block of the
// eigensolver comes from a counter-based device generator instead of torch's Philox stream (the converged factors agree
// to the solver tolerance).
#include "pk_common.h"
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <random>
#include <string>
#include <type_traits>
#include <vector>

// The machine constants of the cost models, ONE table (the split decision of a sharded product and the choice of
// method / block width must not drift between copies — every rank derives its sequence of collectives from them).  The Python
// layer reads the same numbers from polara_amd/machine_model.py; tests/test_host_logic.py compares the two tables.
namespace model {
constexpr double kDenseF64Flops = 20e12;          // dense_f64_flops
constexpr double kLanczosStepFixedS = 0.3e-3;     // lanczos_step_fixed_s
constexpr double kNestedSolveS = 1.5e-3;          // nested_solve_s
constexpr double kXgmiBusBps = 100e9;             // xgmi_bus_Bps (ASSUMED: no N > 1 run exists)
constexpr double kCollectiveStepS = 5e-6;         // collective_step_s (ASSUMED likewise)
}  // namespace model

// Device memory of a context: freed blocks are kept and handed out again (best fit within 25 %): every buffer of the
// solver lives for a few launches on the context's ONE stream, so reuse is stream-ordered and a build does not pay a
// hipMalloc / hipFree (each a device synchronisation) per temporary.
struct DevPool {
    std::multimap<size_t, void *> free_blocks;
    void *get(size_t &bytes) {          // may hand out a larger block: `bytes` becomes its size
        auto it = free_blocks.lower_bound(bytes);
        if (it != free_blocks.end() && it->first <= bytes + bytes / 4 + 4096) {
            void *p = it->second;
            bytes = it->first;
            free_blocks.erase(it);
            return p;
        }
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            trim();                                   // give the cached blocks back and try once more
            if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        }
        return p;
    }
    void put(void *p, size_t bytes) { free_blocks.emplace(bytes, p); }
    void trim() {
        for (auto &kv : free_blocks) (void)hipFree(kv.second);
        free_blocks.clear();
    }
};

// What a host may choose about the builds of a context (pk_ctx_set_option): explicit calls, not environment variables.
struct CtxOptions {
    int svd_method = 0;      // 0 = the cost model (svd_build_impl), 1 = block Lanczos, 2 = filtered subspace iteration
    int krylov_block = 0;    // 0 = the cost model (choose_krylov_block), else the width of a Krylov block
    int dist_overlap = 1;    // two-panel exchange of a sharded product: 0 = never, 1 = by the cost model, 2 = whenever possible
    int hooi_ttm = 0;        // 1 = the per-entry mode products (pk_ttm_f64) instead of the factored form
    int time_spmm = 0;       // 1 = HIP events around every SpMM launch of this context's builds (pk_ctx_spmm_timings: bench.py's roofline of the build)
};

struct SpmmTiming {
    hipEvent_t e0, e1;
    int64_t meta[6];         // rows written, rows gathered from, entries, columns, bytes per stored value, bytes per element of the dense block
};

struct pk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string err;
    DevPool pool;
    CtxOptions opt;
    std::vector<SpmmTiming> spmm_timings;
    std::vector<hipEvent_t> event_pool;      // events of collected timings, handed out again (hipEventCreate costs tens of microseconds)
};

static thread_local DevPool *g_pool = nullptr;   // the pool of the context whose call runs on this thread
struct PoolScope {
    DevPool *prev;
    explicit PoolScope(pk_ctx *ctx) : prev(g_pool) { g_pool = &ctx->pool; }
    ~PoolScope() { g_pool = prev; }
};

namespace {

int fail(pk_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    pk_set_error("%s", buf);
    return code;
}
#define CK(call)                                                          \
    do {                                                                  \
        int rc_ = (call);                                                 \
        if (rc_ != PK_OK) {                                               \
            ctx->err = pk_last_error();                                   \
            return rc_;                                                   \
        }                                                                 \
    } while (0)
#define HIPCK(call)                                                                              \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return fail(ctx, PK_E_LAUNCH, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

struct Dev {   // one device allocation (from the calling context's pool)
    void *p = nullptr;
    size_t bytes = 0;
    size_t cap = 0;
    DevPool *pool = nullptr;
    bool borrowed = false;      // memory of the caller (pk_mat_wrap_device, the views of pk_lanczos_steps): never freed here
    Dev() {}
    explicit Dev(size_t b) { alloc(b); }
    Dev(const Dev &) = delete;
    Dev &operator=(const Dev &) = delete;
    Dev(Dev &&o) noexcept : p(o.p), bytes(o.bytes), cap(o.cap), pool(o.pool), borrowed(o.borrowed) { o.p = nullptr; o.bytes = o.cap = 0; o.borrowed = false; }
    Dev &operator=(Dev &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p; bytes = o.bytes; cap = o.cap; pool = o.pool; borrowed = o.borrowed; o.p = nullptr; o.bytes = o.cap = 0; o.borrowed = false;
        }
        return *this;
    }
    void borrow(const void *ptr, size_t b) {
        release();
        p = const_cast<void *>(ptr); bytes = b; cap = 0; pool = nullptr; borrowed = true;
    }
    ~Dev() { release(); }
    bool alloc(size_t b) {
        release();
        bytes = b;
        if (b == 0) return true;
        pool = g_pool;
        cap = ((b + 65535) / 65536) * 65536;
        if (pool) p = pool->get(cap);
        else if (hipMalloc(&p, cap) != hipSuccess) p = nullptr;
        if (!p) { bytes = cap = 0; return false; }
        return true;
    }
    void release() {
        if (p && !borrowed) {
            if (pool) pool->put(p, cap); else (void)hipFree(p);
        }
        p = nullptr;
        borrowed = false;
        bytes = cap = 0;
    }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct DMat {   // dense row-major fp64 [n x l], contiguous
    Dev buf;
    int64_t n = 0;
    int l = 0;
    DMat() {}
    DMat(int64_t n_, int l_) : buf((size_t)std::max<int64_t>(n_, 1) * std::max(l_, 1) * 8), n(n_), l(l_) {}
    static DMat view(const double *ptr, int64_t n_, int l_) {      // a contiguous [n x l] block of the caller's memory
        DMat m;
        m.buf.borrow(ptr, (size_t)n_ * l_ * 8);
        m.n = n_; m.l = l_;
        return m;
    }
    double *p() const { return buf.as<double>(); }
    bool ok() const { return buf.p != nullptr; }
};

struct Plan {
    Dev task_row, task_begin, task_end, task_slot, long_row, long_sb, long_se, row_first_task, row_long_index, partial;
    int64_t n_tasks = 0, n_long = 0, n_slots = 0;
    bool built = false;
};

struct Csr {
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    int val_kind = PK_VAL_F32;
    Dev indptr, indices, values;
    Plan plan;
};

struct Range { int64_t t0, nt, l0, nl; };

__global__ void transpose_small_kernel(int n, const double *__restrict__ in, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * n) return;
    const int r = i / n, c = i - r * n;
    out[(int64_t)c * n + r] = in[i];
}

// fp32 image of a contiguous fp64 block (the rounded products of the late Lanczos steps gather half the bytes)
__global__ void f64_to_f32_kernel(int64_t n, const double *__restrict__ in, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}

__global__ void unit_block_kernel(int64_t n, int l, double *__restrict__ out) {     // out[n x l] = first l unit vectors
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * l) return;
    const int64_t r = i / l;
    out[i] = (r == i - r * l) ? 1.0 : 0.0;
}

// H <- (H + H^T) / 2 (out of place): a Rayleigh-Ritz matrix X^T (T X) is symmetric to rounding only
__global__ void symmetrize_kernel(int n, const double *__restrict__ in, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * n) return;
    const int r = i / n, c = i - r * n;
    out[i] = 0.5 * (in[i] + in[(int64_t)c * n + r]);
}

// fp32 image of the item factors for the approximate fold-in: columns 0..K-1 = fl32(V), column K = the row-norm bound
__global__ void v32_image_kernel(int64_t n, int K, int ld32, const double *__restrict__ V, const float *__restrict__ bound,
                                 float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * ld32) return;
    const int64_t r = i / ld32;
    const int c = (int)(i - r * ld32);
    out[i] = c < K ? (float)V[r * K + c] : (c == K ? bound[r] : 0.0f);
}

// standard normal start block: counter-based (pk_mix64 of seed and element index -> two uniforms -> Box-Muller), so
// the block depends on (seed, n, l) only — no host generator, no 14 MB upload
__global__ void randn_kernel(int64_t n_elems, uint64_t seed, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_elems) return;
    const uint64_t a = pk_mix64(seed * 0xD1342543DE82EF95ull + (uint64_t)(2 * i));
    const uint64_t b = pk_mix64(seed * 0xD1342543DE82EF95ull + (uint64_t)(2 * i + 1));
    const double u1 = ((double)(a >> 11) + 1.0) * (1.0 / 9007199254740993.0);     // (0, 1)
    const double u2 = (double)(b >> 11) * (1.0 / 9007199254740992.0);             // [0, 1)
    out[i] = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

__global__ void transpose_kernel(int64_t n, int m, const double *__restrict__ in, double *__restrict__ out) {   // [n x m] -> [m x n]
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * m) return;
    const int64_t r = i / m;
    const int c = (int)(i - r * m);
    out[(int64_t)c * n + r] = in[i];
}

__global__ void iota_i32_kernel(int64_t n, int32_t *out, int32_t *count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int32_t)i;
    if (i == 0 && count) *count = (int32_t)n;
}

}  // namespace

struct pk_mat {
    Csr A;
    std::unique_ptr<Csr> Tb;          // user-blocked transpose image
    int64_t rows_per_block = 0, n_blocks = 0;
    std::vector<Range> block_ranges;
    std::vector<int64_t> block_nnz;
    bool nonneg = true;
};

namespace {

int build_plan(pk_ctx *ctx, Csr &M, int split = 1024) {
    if (M.plan.built) return PK_OK;
    hipStream_t st = ctx->stream;
    Dev work((size_t)pk_row_plan_work_bytes(M.n_rows)), counts(3 * 8);
    if (!work.p || !counts.p) return fail(ctx, PK_E_LAUNCH, "out of device memory (row plan)");
    CK(pk_row_plan_count(st, M.n_rows, M.indptr.as<int64_t>(), split, counts.as<int64_t>(), work.p));
    int64_t h[3];
    HIPCK(hipMemcpyAsync(h, counts.p, 24, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    Plan &P = M.plan;
    P.n_tasks = h[0]; P.n_long = h[1]; P.n_slots = h[2];
    const size_t nt = (size_t)std::max<int64_t>(P.n_tasks, 1), nl = (size_t)std::max<int64_t>(P.n_long, 1);
    if (!P.task_row.alloc(nt * 4) || !P.task_begin.alloc(nt * 8) || !P.task_end.alloc(nt * 8) || !P.task_slot.alloc(nt * 4) ||
        !P.long_row.alloc(nl * 4) || !P.long_sb.alloc(nl * 4) || !P.long_se.alloc(nl * 4) ||
        !P.row_first_task.alloc((size_t)(M.n_rows + 1) * 8) || !P.row_long_index.alloc((size_t)(M.n_rows + 1) * 8))
        return fail(ctx, PK_E_LAUNCH, "out of device memory (row plan arrays)");
    CK(pk_row_plan_fill(st, M.n_rows, M.indptr.as<int64_t>(), work.p, P.task_row.as<int32_t>(), P.task_begin.as<int64_t>(),
                        P.task_end.as<int64_t>(), P.task_slot.as<int32_t>(), P.long_row.as<int32_t>(), P.long_sb.as<int32_t>(),
                        P.long_se.as<int32_t>(), P.row_first_task.as<int64_t>(), P.row_long_index.as<int64_t>()));
    HIPCK(hipStreamSynchronize(st));   // `work` dies with this scope
    P.built = true;
    return PK_OK;
}

int task_range(pk_ctx *ctx, Csr &M, int64_t lo, int64_t hi, Range *out) {
    int64_t t[2], l[2];
    hipStream_t st = ctx->stream;
    HIPCK(hipMemcpyAsync(&t[0], M.plan.row_first_task.as<int64_t>() + lo, 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(&t[1], M.plan.row_first_task.as<int64_t>() + hi, 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(&l[0], M.plan.row_long_index.as<int64_t>() + lo, 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(&l[1], M.plan.row_long_index.as<int64_t>() + hi, 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    *out = Range{t[0], t[1] - t[0], l[0], l[1] - l[0]};
    return PK_OK;
}

// out[.. x nc] (+)= M X over the plan slice `rg`
int spmm(pk_ctx *ctx, Csr &M, const void *X, int x_kind, int64_t ldx, int nc, double *out, int64_t ldo, const Range &rg,
         int64_t row_base = 0, int accumulate = 0, const int64_t *shape3 = nullptr) {
    Plan &P = M.plan;
    const size_t xe = x_kind == PK_VAL_F64 ? 8 : 4;
    for (int c0 = 0; c0 < nc; c0 += 256) {
        const int w = std::min(256, nc - c0);
        const size_t need = (size_t)P.n_slots * w * 8;
        if (need > P.partial.bytes && !P.partial.alloc(need)) return fail(ctx, PK_E_LAUNCH, "out of device memory (spmm partials)");
        SpmmTiming tm;
        if (ctx->opt.time_spmm) {
            auto take = [&](hipEvent_t *e) -> hipError_t {
                if (!ctx->event_pool.empty()) { *e = ctx->event_pool.back(); ctx->event_pool.pop_back(); return hipSuccess; }
                return hipEventCreate(e);
            };
            HIPCK(take(&tm.e0));
            HIPCK(take(&tm.e1));
            const int64_t whole[3] = {M.n_rows, M.n_cols, M.nnz};
            const int64_t *sh = shape3 ? shape3 : whole;
            tm.meta[0] = sh[0]; tm.meta[1] = sh[1]; tm.meta[2] = sh[2]; tm.meta[3] = w;
            tm.meta[4] = M.val_kind == PK_VAL_F32 ? 4 : 8; tm.meta[5] = (int64_t)xe;
            HIPCK(hipEventRecord(tm.e0, ctx->stream));
        }
        CK(pk_spmm_csr_ex(ctx->stream, rg.nt, P.task_row.as<int32_t>() + rg.t0, P.task_begin.as<int64_t>() + rg.t0,
                          P.task_end.as<int64_t>() + rg.t0, P.task_slot.as<int32_t>() + rg.t0, rg.nl,
                          P.long_row.as<int32_t>() + rg.l0, P.long_sb.as<int32_t>() + rg.l0, P.long_se.as<int32_t>() + rg.l0,
                          M.indices.as<int32_t>(), M.values.p, M.val_kind, static_cast<const char *>(X) + (size_t)c0 * xe, x_kind, ldx,
                          w, out + c0, ldo, P.partial.as<double>(), row_base, accumulate, M.n_cols));      // (x_rows: the dense block has one row per column of M — lets the launcher take 32-bit row offsets)
        if (ctx->opt.time_spmm) {
            HIPCK(hipEventRecord(tm.e1, ctx->stream));
            ctx->spmm_timings.push_back(tm);
        }
    }
    return PK_OK;
}

int spmm_full(pk_ctx *ctx, Csr &M, const DMat &X, DMat &out) {
    return spmm(ctx, M, X.p(), PK_VAL_F64, X.l, X.l, out.p(), out.l, Range{0, M.plan.n_tasks, 0, M.plan.n_long});
}

// nc: the width of the blocks the image will multiply — a user block's rows of Y (nc fp64 columns) are meant to stay in the L2s
// (8 MB at 16 384 rows of 64 columns), so a narrow Krylov block takes proportionally more users per launch (round 6: eight
// launches of A^T Y per step at b = 16 were four fifths launch overhead)
int ensure_blocked_transpose(pk_ctx *ctx, pk_mat *m, int nc = 64) {
    if (m->Tb) return PK_OK;
    Csr &A = m->A;
    const int64_t l2_rows = 16384 * (int64_t)std::max(1, 64 / std::max(16, std::min(nc, 64)));
    int64_t rpb = std::max<int64_t>(l2_rows, (int64_t)(64.0 * (double)A.n_cols * (double)A.n_rows / (double)std::max<int64_t>(A.nnz, 1)));
    rpb = ((rpb + 4095) / 4096) * 4096;
    rpb = std::min<int64_t>(rpb, std::max<int64_t>(A.n_rows, 1));
    if (A.n_rows < 2 * 16384) rpb = std::max<int64_t>(A.n_rows, 1);          // small matrices: one block = the plain transpose
    const int64_t nb = (A.n_rows + rpb - 1) / rpb;
    auto T = std::make_unique<Csr>();
    T->n_rows = nb * A.n_cols; T->n_cols = A.n_rows; T->nnz = A.nnz; T->val_kind = A.val_kind;
    const size_t ve = A.val_kind == PK_VAL_F32 ? 4 : 8;
    if (!T->indptr.alloc((size_t)(T->n_rows + 1) * 8) || !T->indices.alloc((size_t)std::max<int64_t>(A.nnz, 1) * 4) ||
        !T->values.alloc((size_t)std::max<int64_t>(A.nnz, 1) * ve))
        return fail(ctx, PK_E_LAUNCH, "out of device memory (transpose)");
    Dev work((size_t)pk_csr_transpose_work_bytes(A.nnz));
    if (!work.p) return fail(ctx, PK_E_LAUNCH, "out of device memory (transpose work)");
    CK(pk_csr_transpose(ctx->stream, A.n_rows, A.n_cols, A.nnz, A.indptr.as<int64_t>(), A.indices.as<int32_t>(), A.values.p,
                        A.val_kind, nb > 1 ? rpb : 0, T->indptr.as<int64_t>(), T->indices.as<int32_t>(), T->values.p, work.p));
    HIPCK(hipStreamSynchronize(ctx->stream));
    CK(build_plan(ctx, *T));
    m->block_ranges.resize((size_t)nb);
    for (int64_t b = 0; b < nb; ++b) CK(task_range(ctx, *T, b * A.n_cols, (b + 1) * A.n_cols, &m->block_ranges[(size_t)b]));
    {   // entries per block (the timing records of bench.py's build roofline)
        std::vector<int64_t> edges((size_t)nb + 1);
        for (int64_t b = 0; b <= nb; ++b)
            HIPCK(hipMemcpyAsync(&edges[(size_t)b], T->indptr.as<int64_t>() + b * A.n_cols, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCK(hipStreamSynchronize(ctx->stream));
        m->block_nnz.resize((size_t)nb);
        for (int64_t b = 0; b < nb; ++b) m->block_nnz[(size_t)b] = edges[(size_t)b + 1] - edges[(size_t)b];
    }
    m->rows_per_block = rpb; m->n_blocks = nb;
    m->Tb = std::move(T);
    return PK_OK;
}

// Z = A^T Y, user block by user block (block b > 0 adds)
int spmm_t(pk_ctx *ctx, pk_mat *m, const DMat &Y, DMat &Z) {
    for (int64_t b = 0; b < m->n_blocks; ++b) {
        const int64_t shape3[3] = {b == 0 ? m->A.n_cols : 0, m->rows_per_block, m->block_nnz[(size_t)b]};
        CK(spmm(ctx, *m->Tb, Y.p(), PK_VAL_F64, Y.l, Y.l, Z.p(), Z.l, m->block_ranges[(size_t)b], b * m->A.n_cols, b > 0, shape3));
    }
    return PK_OK;
}

// Z [n_cols x w] = A^T Y[:, c0 : c0 + w]: one column panel of the product (the panels of GramianOp::apply)
int spmm_t_cols(pk_ctx *ctx, pk_mat *m, const DMat &Y, int c0, int w, DMat &Z) {
    for (int64_t b = 0; b < m->n_blocks; ++b)
        CK(spmm(ctx, *m->Tb, Y.p() + c0, PK_VAL_F64, Y.l, w, Z.p(), Z.l, m->block_ranges[(size_t)b], b * m->A.n_cols, b > 0));
    return PK_OK;
}

// ---- dense helpers (each returns a fresh matrix through `out`) -------------------------------------------------------
struct Solver {
    pk_ctx *ctx;
    hipStream_t st;
    Dev gram_work;

    int gram(const DMat &A, const DMat &B, DMat &G) {
        G = DMat(A.l, B.l);
        const size_t need = (size_t)pk_gram_work_bytes(A.n, A.l, B.l);
        if (need > gram_work.bytes && !gram_work.alloc(need)) return fail(ctx, PK_E_LAUNCH, "out of device memory (gram)");
        CK(pk_gram_f64(st, A.n, A.l, B.l, A.p(), A.l, B.p(), B.l, G.p(), G.l, gram_work.p));
        return PK_OK;
    }
    int tsmm(const DMat &X, const DMat &C, DMat &out) {
        out = DMat(X.n, C.l);
        if (!out.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (tsmm)");
        CK(pk_tsmm_f64(st, X.n, X.l, C.l, X.p(), X.l, C.p(), C.l, out.p(), out.l));
        return PK_OK;
    }
    int tsmm_axpby(const DMat &X, const DMat &C, double a, double b, const DMat *Z1, double c, const DMat *Z2, DMat &out) {
        out = DMat(X.n, C.l);       // out = a X C + b Z1 + c Z2 in one launch
        if (!out.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (tsmm_axpby)");
        CK(pk_tsmm_axpby_f64(st, X.n, X.l, C.l, X.p(), X.l, C.p(), C.l, a, b, Z1 ? Z1->p() : nullptr, Z1 ? Z1->l : 0, c,
                             Z2 ? Z2->p() : nullptr, Z2 ? Z2->l : 0, out.p(), out.l));
        return PK_OK;
    }
    int axpbypcz(double a, const DMat &Z, double b, const DMat *Y, double c, const DMat *X, DMat &out) {
        out = DMat(Z.n, Z.l);
        if (!out.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (axpbypcz)");
        CK(pk_axpbypcz_f64(st, Z.n * Z.l, a, Z.p(), b, Y ? Y->p() : nullptr, c, X ? X->p() : nullptr, out.p()));
        return PK_OK;
    }
    int project_out(const DMat &X, const DMat &V, DMat &out) {   // X - V (V^T X)
        DMat G, T;
        CK(gram(V, X, G));
        CK(tsmm(V, G, T));
        return axpbypcz(1.0, X, -1.0, &T, 0.0, nullptr, out);
    }
    int to_host(const void *dev, void *host, size_t bytes) {
        HIPCK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        return PK_OK;
    }
    int upload(const void *host, void *dev, size_t bytes) {
        HIPCK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st));
        HIPCK(hipStreamSynchronize(st));
        return PK_OK;
    }
    // eigen-decomposition of a small PSD matrix: lam (host, descending), C (device, COLUMN j = j-th eigenvector)
    int eigh(const DMat &S, std::vector<double> &lam, DMat &C, Dev &lam_dev) {
        const int n = S.l;
        DMat W(n, n), R(n, n);
        Dev info(8);
        if (!lam_dev.alloc((size_t)n * 8) || !W.ok() || !R.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (eigh)");
        HIPCK(hipMemcpyAsync(W.p(), S.p(), (size_t)n * n * 8, hipMemcpyDeviceToDevice, st));
        CK(pk_eigh_psd_f64(st, n, W.p(), n, R.p(), n, lam_dev.as<double>(), 0, 0.0, info.as<int32_t>()));
        if (n > 136) {
            // block Jacobi (one cooperative launch with grid barriers): a verdict of 0 — a barrier that did not complete,
            // or sweeps that ran out — must not hand half-rotated vectors on: re-do launch by launch
            int32_t verdict[2] = {0, 0};
            CK(to_host(info.p, verdict, sizeof verdict));
            if (verdict[1] == 0) {
                HIPCK(hipMemcpyAsync(W.p(), S.p(), (size_t)n * n * 8, hipMemcpyDeviceToDevice, st));
                CK(pk_eigh_psd_rounds_f64(st, n, W.p(), n, R.p(), n, lam_dev.as<double>(), 0, 0.0, info.as<int32_t>()));
                CK(to_host(info.p, verdict, sizeof verdict));
                if (verdict[1] == 0) return fail(ctx, PK_E_LAUNCH, "eigh: the block Jacobi sweeps did not converge (n=%d)", n);
            }
        }
        C = DMat(n, n);
        hipLaunchKernelGGL(transpose_small_kernel, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, n, R.p(), C.p());
        lam.resize((size_t)n);
        return to_host(lam_dev.p, lam.data(), (size_t)n * 8);
    }
    int col_slice(const DMat &X, int c0, int c1, DMat &out) {
        out = DMat(X.n, c1 - c0);
        if (!out.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (col_slice)");
        HIPCK(hipMemcpy2DAsync(out.p(), (size_t)(c1 - c0) * 8, X.p() + c0, (size_t)X.l * 8, (size_t)(c1 - c0) * 8, (size_t)X.n,
                               hipMemcpyDeviceToDevice, st));
        return PK_OK;
    }
    int hcat(const DMat *A, const DMat &B, DMat &out) {
        const int la = A ? A->l : 0;
        out = DMat(B.n, la + B.l);
        if (!out.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (hcat)");
        if (A) HIPCK(hipMemcpy2DAsync(out.p(), (size_t)out.l * 8, A->p(), (size_t)la * 8, (size_t)la * 8, (size_t)B.n, hipMemcpyDeviceToDevice, st));
        HIPCK(hipMemcpy2DAsync(out.p() + la, (size_t)out.l * 8, B.p(), (size_t)B.l * 8, (size_t)B.l * 8, (size_t)B.n, hipMemcpyDeviceToDevice, st));
        return PK_OK;
    }
    int randn(int64_t n, int l, uint64_t seed, DMat &out) {
        out = DMat(n, l);
        if (!out.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (randn)");
        const int64_t ne = n * l;
        hipLaunchKernelGGL(randn_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, ne, seed, out.p());
        return PK_OK;
    }
    int scale_cols_host(DMat &X, const std::vector<double> &s) {
        Dev sd(s.size() * 8);
        if (!sd.p) return fail(ctx, PK_E_LAUNCH, "out of device memory (scale)");
        CK(upload(s.data(), sd.p, s.size() * 8));
        CK(pk_scale_cols_f64(st, X.n, X.l, X.p(), X.l, sd.as<double>()));
        HIPCK(hipStreamSynchronize(st));
        return PK_OK;
    }
    // orthonormal basis of span(X) (orthogonal to Vlock) by eigen-whitening, `passes` times (solver._whiten)
    int whiten(DMat &X, const DMat *Vlock, int passes) {
        for (int p = 0; p < passes; ++p) {
            if (Vlock && Vlock->l > 0) { DMat t; CK(project_out(X, *Vlock, t)); X = std::move(t); }
            DMat G, C, Y;
            std::vector<double> lam;
            Dev lam_dev;
            CK(gram(X, X, G));
            CK(eigh(G, lam, C, lam_dev));
            std::vector<double> s(lam.size());
            const double floor_ = std::max(1e-300, lam.empty() ? 0.0 : lam[0] * 1e-30);
            for (size_t i = 0; i < lam.size(); ++i) s[i] = 1.0 / std::sqrt(std::max(lam[i], floor_));
            CK(scale_cols_host(C, s));
            CK(tsmm(X, C, Y));
            X = std::move(Y);
        }
        return PK_OK;
    }
    // solver._refill: basis of the numerical range of X completed by fresh random vectors
    int refill(const DMat &X0, const DMat *Vlock, uint64_t seed, DMat &out) {
        DMat X;
        if (Vlock && Vlock->l > 0) CK(project_out(X0, *Vlock, X)); else CK(col_slice(X0, 0, X0.l, X));
        DMat G, C;
        std::vector<double> lam;
        Dev lam_dev;
        CK(gram(X, X, G));
        CK(eigh(G, lam, C, lam_dev));
        int ng = 0;
        if (!lam.empty() && lam[0] > 0) for (double v : lam) ng += v > lam[0] * 1e-20;
        DMat good;
        if (ng) {
            DMat Cg, Xg;
            CK(col_slice(C, 0, ng, Cg));
            std::vector<double> s((size_t)ng);
            for (int i = 0; i < ng; ++i) s[(size_t)i] = 1.0 / std::sqrt(lam[(size_t)i]);
            CK(scale_cols_host(Cg, s));
            CK(tsmm(X, Cg, Xg));
            CK(whiten(Xg, Vlock, 1));
            good = std::move(Xg);
        }
        if (ng < X.l) {
            DMat R;
            CK(randn(X.n, X.l - ng, seed, R));
            for (int it = 0; it < 2; ++it) {
                if (ng) { DMat t; CK(project_out(R, good, t)); R = std::move(t); }
                CK(whiten(R, Vlock, 1));
            }
            if (ng) CK(hcat(&good, R, out)); else out = std::move(R);
        } else {
            out = std::move(good);
        }
        return PK_OK;
    }
    // solver.orthonormalize: shifted CholeskyQR3, verified; rank-deficient blocks go to refill
    int orthonormalize(const DMat &X, const DMat *Vlock, uint64_t seed, DMat &out) {
        const int64_t m = X.n;
        const int l = X.l;
        const double u = 1.1102230246251565e-16;
        Dev info(3 * 4);
        if (!info.p) return fail(ctx, PK_E_LAUNCH, "out of device memory");
        HIPCK(hipMemsetAsync(info.p, 0, 12, st));
        DMat Y;
        CK(col_slice(X, 0, l, Y));
        Dev chol_work((size_t)std::max<int64_t>(pk_chol_work_bytes(l), 8));
        for (int p = 0; p < 3; ++p) {
            if (Vlock && Vlock->l > 0) { DMat t; CK(project_out(Y, *Vlock, t)); Y = std::move(t); }
            DMat G, Rinv(l, l), Yn;
            CK(gram(Y, Y, G));
            CK(pk_chol_rinv_f64(st, l, G.p(), l, p == 0 ? 11.0 * ((double)m * l + (double)l * (l + 1)) * u : 0.0, Rinv.p(), l,
                                chol_work.p, info.as<int32_t>() + p));
            CK(tsmm(Y, Rinv, Yn));
            Y = std::move(Yn);
        }
        DMat G;
        CK(gram(Y, Y, G));
        std::vector<double> g((size_t)l * l);
        int32_t inf[3];
        CK(to_host(G.p(), g.data(), g.size() * 8));
        CK(to_host(info.p, inf, 12));
        double err = 0.0;
        for (int i = 0; i < l; ++i)
            for (int j = 0; j < l; ++j) err = std::max(err, std::fabs(g[(size_t)i * l + j] - (i == j ? 1.0 : 0.0)));
        if (inf[0] || inf[1] || inf[2] || !(err < 1e-8)) return refill(X, Vlock, seed, out);
        out = std::move(Y);
        return PK_OK;
    }
    int resid(const DMat &Z, const DMat &X, const Dev &theta_dev, std::vector<double> &res) {
        const int nb = pk_resid_blocks(Z.n);
        Dev part((size_t)nb * Z.l * 8);
        if (!part.p) return fail(ctx, PK_E_LAUNCH, "out of device memory (resid)");
        CK(pk_resid_colnorm2_f64(st, Z.n, Z.l, Z.p(), Z.l, X.p(), X.l, theta_dev.as<double>(), part.as<double>()));
        std::vector<double> h((size_t)nb * Z.l);
        CK(to_host(part.p, h.data(), h.size() * 8));
        res.assign((size_t)Z.l, 0.0);
        for (int b = 0; b < nb; ++b)
            for (int j = 0; j < Z.l; ++j) res[(size_t)j] += h[(size_t)b * Z.l + j];
        for (auto &v : res) v = std::sqrt(std::max(v, 0.0));
        return PK_OK;
    }
};

int cheb_degree(double theta_top, double b, double spread, int m_max) {
    if (b <= 0.0) return 2;
    const double x_top = 2.0 * theta_top / b - 1.0;
    if (x_top <= 1.0 + 1e-12) return m_max;
    const int m = (int)(std::log(2.0 * spread) / std::acosh(x_top));
    return std::max(2, std::min(m_max, m));
}

int upload_csr(pk_ctx *ctx, Csr &M, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *indptr, const int32_t *indices,
               const void *values, int val_kind) {
    M.n_rows = n_rows; M.n_cols = n_cols; M.nnz = nnz; M.val_kind = val_kind;
    const size_t ve = val_kind == PK_VAL_F32 ? 4 : 8;
    if (!M.indptr.alloc((size_t)(n_rows + 1) * 8) || !M.indices.alloc((size_t)std::max<int64_t>(nnz, 1) * 4) ||
        !M.values.alloc((size_t)std::max<int64_t>(nnz, 1) * ve))
        return fail(ctx, PK_E_LAUNCH, "out of device memory (matrix)");
    HIPCK(hipMemcpyAsync(M.indptr.p, indptr, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (nnz) {
        HIPCK(hipMemcpyAsync(M.indices.p, indices, (size_t)nnz * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCK(hipMemcpyAsync(M.values.p, values, (size_t)nnz * ve, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCK(hipStreamSynchronize(ctx->stream));
    return PK_OK;
}

}  // namespace

// ============================================================================================================
extern "C" int pk_ctx_create(int32_t device, pk_ctx **out) {
    if (!out) return PK_E_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        pk_set_error("pk_ctx_create: device %d not available (%d visible)", device, n);
        return PK_E_LAUNCH;
    }
    auto *ctx = new pk_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&ctx->stream) != hipSuccess) {
        delete ctx;
        pk_set_error("pk_ctx_create: cannot create a stream on device %d", device);
        return PK_E_LAUNCH;
    }
    // every code object of the library is loaded now, not inside the first build of this context (api.cpp)
    if (pk_warm_up() != PK_OK) {
        (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return PK_E_LAUNCH;
    }
    *out = ctx;
    return PK_OK;
}

extern "C" void pk_ctx_destroy(pk_ctx *ctx) {
    if (!ctx) return;
    for (auto &t : ctx->spmm_timings) { (void)hipEventDestroy(t.e0); (void)hipEventDestroy(t.e1); }
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    ctx->spmm_timings.clear();
    ctx->event_pool.clear();
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->pool.trim();
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" const char *pk_ctx_error(pk_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" int pk_ctx_set_option(pk_ctx *ctx, const char *name, int32_t value) {
    if (!ctx || !name) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    struct { const char *name; int *slot; int lo, hi; } table[] = {
        {"svd_method", &ctx->opt.svd_method, 0, 2},   {"krylov_block", &ctx->opt.krylov_block, 0, 1024},
        {"dist_overlap", &ctx->opt.dist_overlap, 0, 2}, {"hooi_ttm", &ctx->opt.hooi_ttm, 0, 1}, {"time_spmm", &ctx->opt.time_spmm, 0, 1}};
    for (auto &e : table)
        if (!strcmp(name, e.name)) {
            if (value < e.lo || value > e.hi) return fail(ctx, PK_E_INVALID, "pk_ctx_set_option: %s takes %d..%d", name, e.lo, e.hi);
            *e.slot = value;
            return PK_OK;
        }
    return fail(ctx, PK_E_INVALID, "pk_ctx_set_option: unknown option '%s'", name);
}

// the SpMM launches recorded since the last call (option "time_spmm"): waits for them, writes min(count, cap) records —
// ms_out[i] = duration, meta_out[6 i ..] = {rows written, rows gathered from, entries, columns, bytes per stored value, bytes per
// element of the dense block} — forgets them all, returns the count
extern "C" int64_t pk_ctx_spmm_timings(pk_ctx *ctx, double *ms_out, int64_t *meta_out, int64_t cap) {
    if (!ctx) return -1;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    const int64_t count = (int64_t)ctx->spmm_timings.size();
    for (int64_t i = 0; i < count; ++i) {
        SpmmTiming &t = ctx->spmm_timings[(size_t)i];
        float ms = 0.f;
        (void)hipEventSynchronize(t.e1);
        (void)hipEventElapsedTime(&ms, t.e0, t.e1);
        if (i < cap && ms_out && meta_out) {
            ms_out[i] = (double)ms;
            for (int q = 0; q < 6; ++q) meta_out[6 * i + q] = t.meta[q];
        }
        ctx->event_pool.push_back(t.e0);
        ctx->event_pool.push_back(t.e1);
    }
    ctx->spmm_timings.clear();
    return count;
}

extern "C" int pk_mat_from_csr(pk_ctx *ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *indptr,
                               const int32_t *indices, const void *values, int32_t val_kind, pk_mat **out) {
    if (!ctx || !out) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    (void)hipSetDevice(ctx->device);
    if (n_rows < 1 || n_cols < 1 || nnz < 0 || !indptr || (nnz && (!indices || !values)) ||
        (val_kind != PK_VAL_F32 && val_kind != PK_VAL_F64))
        return fail(ctx, PK_E_INVALID, "pk_mat_from_csr: bad arguments");
    if (indptr[0] != 0 || indptr[n_rows] != nnz) return fail(ctx, PK_E_INVALID, "pk_mat_from_csr: indptr does not span [0, nnz]");
    for (int64_t p = 0; p < nnz; ++p)
        if (indices[p] < 0 || indices[p] >= n_cols) return fail(ctx, PK_E_INVALID, "pk_mat_from_csr: column index out of bounds");
    auto m = std::make_unique<pk_mat>();
    int rc = upload_csr(ctx, m->A, n_rows, n_cols, nnz, indptr, indices, values, val_kind);
    if (rc != PK_OK) return rc;
    m->nonneg = true;
    if (val_kind == PK_VAL_F32) { const float *v = static_cast<const float *>(values); for (int64_t p = 0; p < nnz; ++p) if (v[p] < 0) { m->nonneg = false; break; } }
    else { const double *v = static_cast<const double *>(values); for (int64_t p = 0; p < nnz; ++p) if (v[p] < 0) { m->nonneg = false; break; } }
    rc = build_plan(ctx, m->A);
    if (rc != PK_OK) return rc;
    *out = m.release();
    return PK_OK;
}

static int mat_from_coo_impl(pk_ctx *ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *rows, const int64_t *cols,
                             int64_t idx_stride, const void *values, int32_t val_kind, pk_mat **out);

extern "C" int pk_mat_from_coo(pk_ctx *ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *rows, const int64_t *cols,
                               int64_t idx_stride, const void *values, int32_t val_kind, pk_mat **out) {
    if (!ctx || !out) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    (void)hipSetDevice(ctx->device);
    return mat_from_coo_impl(ctx, n_rows, n_cols, nnz, rows, cols, idx_stride, values, val_kind, out);
}

// (the caller holds the context's mutex and pool scope: pk_hooi builds its two unfoldings through this)
static int mat_from_coo_impl(pk_ctx *ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *rows, const int64_t *cols,
                             int64_t idx_stride, const void *values, int32_t val_kind, pk_mat **out) {
    if (n_rows < 1 || n_cols < 1 || nnz < 0 || idx_stride < 1 || (nnz && (!rows || !cols || !values)) ||
        (val_kind != PK_VAL_F32 && val_kind != PK_VAL_F64))
        return fail(ctx, PK_E_INVALID, "pk_mat_from_coo: bad arguments");
    hipStream_t st = ctx->stream;
    const size_t ve = val_kind == PK_VAL_F32 ? 4 : 8, n1 = (size_t)std::max<int64_t>(nnz, 1);
    // the index arrays go up as they lie in host memory: one interleaved block (stride 2) or two plain arrays
    const bool interleaved = idx_stride == 2 && cols == rows + 1;
    Dev idx(interleaved ? n1 * 16 : n1 * 16), vals(n1 * ve), info(16), work((size_t)pk_coo_to_csr_work_bytes(nnz));
    auto m = std::make_unique<pk_mat>();
    Csr &A = m->A;
    A.n_rows = n_rows; A.n_cols = n_cols; A.val_kind = val_kind;
    if (!idx.p || !vals.p || !info.p || !work.p || !A.indptr.alloc((size_t)(n_rows + 1) * 8) || !A.indices.alloc(n1 * 4) || !A.values.alloc(n1 * ve))
        return fail(ctx, PK_E_LAUNCH, "out of device memory (pk_mat_from_coo)");
    const int64_t *r_dev, *c_dev;
    int64_t stride_dev;
    if (nnz) {
        if (interleaved) {
            HIPCK(hipMemcpyAsync(idx.p, rows, (size_t)nnz * 16, hipMemcpyHostToDevice, st));
            r_dev = idx.as<int64_t>(); c_dev = r_dev + 1; stride_dev = 2;
        } else {
            HIPCK(hipMemcpy2DAsync(idx.p, 8, rows, (size_t)idx_stride * 8, 8, (size_t)nnz, hipMemcpyHostToDevice, st));
            HIPCK(hipMemcpy2DAsync(idx.as<int64_t>() + nnz, 8, cols, (size_t)idx_stride * 8, 8, (size_t)nnz, hipMemcpyHostToDevice, st));
            r_dev = idx.as<int64_t>(); c_dev = r_dev + nnz; stride_dev = 1;
        }
        HIPCK(hipMemcpyAsync(vals.p, values, (size_t)nnz * ve, hipMemcpyHostToDevice, st));
    } else {
        r_dev = c_dev = idx.as<int64_t>(); stride_dev = 1;
    }
    CK(pk_coo_to_csr(st, nnz, r_dev, c_dev, stride_dev, vals.p, val_kind, n_rows, n_cols, A.indptr.as<int64_t>(), A.indices.as<int32_t>(),
                     A.values.p, info.as<int64_t>(), reinterpret_cast<int32_t *>(info.as<int64_t>() + 1), work.p));
    int64_t h[2];
    HIPCK(hipMemcpyAsync(h, info.p, 16, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if ((int32_t)(h[1] & 0xffffffff)) return fail(ctx, PK_E_INVALID, "pk_mat_from_coo: index out of bounds");
    A.nnz = h[0];
    m->nonneg = true;
    if (val_kind == PK_VAL_F32) { const float *v = static_cast<const float *>(values); for (int64_t p = 0; p < nnz; ++p) if (v[p] < 0) { m->nonneg = false; break; } }
    else { const double *v = static_cast<const double *>(values); for (int64_t p = 0; p < nnz; ++p) if (v[p] < 0) { m->nonneg = false; break; } }
    int rc = build_plan(ctx, A);
    if (rc != PK_OK) return rc;
    *out = m.release();
    return PK_OK;
}

extern "C" void pk_mat_free(pk_ctx *ctx, pk_mat *m) {
    if (!m) return;
    if (ctx) {
        std::lock_guard<std::mutex> lock(ctx->mu);
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        delete m;                        // its blocks go back to the context's pool
    } else {
        delete m;                        // only valid while the creating context is alive
    }
}

extern "C" int64_t pk_mat_nnz(const pk_mat *m) { return m ? m->A.nnz : -1; }

// ------------------------------------------------------------------------------------------------------------
// pk_svd_build: polara_amd/solver.py::svd_topk restated (models.py:835-855)
// ------------------------------------------------------------------------------------------------------------
static int svd_build_impl(pk_ctx *ctx, pk_mat *A, const pk_comm *comm, int32_t k, int32_t block, double tol, int32_t max_outer,
                          uint64_t seed, double *sigma_out, double *V_out, double *U_out, pk_build_stats *stats_out);

extern "C" int pk_svd_build(pk_ctx *ctx, pk_mat *A, int32_t k, int32_t block, double tol, int32_t max_outer, uint64_t seed,
                            double *sigma_out, double *V_out, double *U_out, pk_build_stats *stats_out) {
    return svd_build_impl(ctx, A, nullptr, k, block, tol, max_outer, seed, sigma_out, V_out, U_out, stats_out);
}

extern "C" int pk_svd_build_sharded(pk_ctx *ctx, pk_mat *A_local, const pk_comm *comm, int32_t k, int32_t block, double tol,
                                    int32_t max_outer, uint64_t seed, double *sigma_out, double *V_out, double *U_out_local,
                                    pk_build_stats *stats_out) {
    if (!comm || comm->world < 1 || comm->rank < 0 || comm->rank >= comm->world || (comm->world > 1 && !comm->allreduce_sum_f64))
        return ctx ? fail(ctx, PK_E_INVALID, "pk_svd_build_sharded: bad communicator") : PK_E_INVALID;
    return svd_build_impl(ctx, A_local, comm->world > 1 ? comm : nullptr, k, block, tol, max_outer, seed, sigma_out, V_out,
                          U_out_local, stats_out);
}

extern "C" void *pk_ctx_stream(pk_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

// ---- the filtered subspace iteration, generic in the operator (solver.py::_subspace_iteration) -----------------------
struct SubspaceOut {
    DMat basis;                          // locked vectors, then the active block
    std::vector<double> lam_all;         // Ritz values of the basis columns
    std::vector<double> res_act;         // residual norms of the active block
    int n_lock = 0, outer = 0;
    bool converged = false;
};

// Op: ritz(X, H, carrier) -> H = X^T B X and a carrier from which B (X C) follows; rotate(carrier, C, Z) -> Z = B X C;
// apply(X, Z) -> Z = B X.  X: orthonormal start block (consumed).
// does the operator offer the Chebyshev step as one launch (DenseOp)?
template <typename T, typename = void>
struct has_filter_step : std::false_type {};
template <typename T>
struct has_filter_step<T, std::void_t<decltype(&T::filter_step)>> : std::true_type {};

template <class Op>
int subspace_iteration(pk_ctx *ctx, Solver &S, Op &op, int k, DMat X, double tol, int max_outer, int m_max, double spread,
                       uint64_t seed, bool even_lock, SubspaceOut &out) {
    DMat Vlock;           // [rows x n_lock]
    bool have_lock = false;
    std::vector<double> lam_lock, theta_host, res_host;
    int n_lock = 0;
    bool done = false;
    for (int it = 0; it < max_outer && !done; ++it) {
        out.outer += 1;
        // ---- Rayleigh-Ritz on the active block
        DMat H, carrier, Cm, Xr, Z;
        CK(op.ritz(X, H, carrier));
        Dev theta_dev;
        CK(S.eigh(H, theta_host, Cm, theta_dev));
        CK(S.tsmm(X, Cm, Xr));
        X = std::move(Xr);
        CK(op.rotate(carrier, Cm, Z));
        CK(S.resid(Z, X, theta_dev, res_host));
        const double lam1 = lam_lock.empty() ? theta_host[0] : lam_lock[0];
        const int need = k - n_lock;
        const double thr = tol * lam1;
        int n_new = 0;
        while (n_new < (int)res_host.size() && res_host[(size_t)n_new] <= thr) ++n_new;
        if (n_new < need && (n_new & 1) && even_lock) --n_new;       // even active width: the paired-column SpMM kernel
        if (n_new >= need) {
            done = true;
            break;
        }
        if (n_new > 0 && X.l - n_new >= std::max(8, need - n_new)) {
            DMat newV, Vl, Xa, Za;
            CK(S.col_slice(X, 0, n_new, newV));
            CK(S.hcat(have_lock ? &Vlock : nullptr, newV, Vl));
            Vlock = std::move(Vl);
            have_lock = true;
            lam_lock.insert(lam_lock.end(), theta_host.begin(), theta_host.begin() + n_new);
            n_lock += n_new;
            CK(S.col_slice(X, n_new, X.l, Xa));
            CK(S.col_slice(Z, n_new, Z.l, Za));
            X = std::move(Xa);
            Z = std::move(Za);
            theta_host.erase(theta_host.begin(), theta_host.begin() + n_new);
            res_host.erase(res_host.begin(), res_host.begin() + n_new);
        }
        // ---- Chebyshev filter on P B P, damping [0, b]
        const double b = theta_host.back(), a0 = theta_host.front();
        const int m = cheb_degree(a0, b, spread, m_max);
        const double e = 0.5 * b, c = 0.5 * b;
        // One filter of degree m from the start block Xs with Zs = B Xs: Yc = p_m(P B P) Xs.
        auto cheb_filter = [&](DMat &Xs, DMat &Zs, DMat &Yc) -> int {
            if (e <= 0.0 || a0 <= c) {
                if (have_lock) CK(S.project_out(Zs, Vlock, Yc)); else Yc = std::move(Zs);
                return PK_OK;
            }
            double sigma = e / (a0 - c);
            const double tau = 2.0 / sigma;
            DMat Zp;
            if (have_lock) CK(S.project_out(Zs, Vlock, Zp)); else Zp = std::move(Zs);
            DMat Xc;
            CK(S.col_slice(Xs, 0, Xs.l, Xc));
            CK(S.axpbypcz(sigma / e, Zp, -c * sigma / e, &Xc, 0.0, nullptr, Yc));
            for (int s = 2; s <= m; ++s) {
                const double sigma_new = 1.0 / (tau - sigma);
                DMat Zc, Yn;
                if constexpr (has_filter_step<Op>::value) {
                    if (!have_lock) {          // product and recurrence in one launch (dense operators)
                        CK(op.filter_step(Yc, 2.0 * sigma_new / e, -2.0 * sigma_new * c / e, -sigma * sigma_new, Xc, Yn));
                        Xc = std::move(Yc);
                        Yc = std::move(Yn);
                        sigma = sigma_new;
                        continue;
                    }
                }
                CK(op.apply(Yc, Zc));
                if (have_lock) { DMat t; CK(S.project_out(Zc, Vlock, t)); Zc = std::move(t); }
                CK(S.axpbypcz(2.0 * sigma_new / e, Zc, -2.0 * sigma_new * c / e, &Yc, -sigma * sigma_new, &Xc, Yn));
                Xc = std::move(Yc);
                Yc = std::move(Yn);
                sigma = sigma_new;
            }
            return PK_OK;
        };
        DMat Yc, Xn;
        {
            DMat Xs = std::move(X), Zs = std::move(Z);
            CK(cheb_filter(Xs, Zs, Yc));
        }
        CK(S.orthonormalize(Yc, have_lock ? &Vlock : nullptr, seed + 1 + (uint64_t)it, Xn));
        X = std::move(Xn);
    }
    CK(S.hcat(have_lock ? &Vlock : nullptr, X, out.basis));
    out.lam_all = lam_lock;
    out.lam_all.insert(out.lam_all.end(), theta_host.begin(), theta_host.end());
    out.res_act = res_host;
    out.n_lock = n_lock;
    out.converged = done;
    return PK_OK;
}

// B = A^T A of the (row-sharded) sparse matrix: solver.py::_Gramian
struct GramianOp {
    pk_ctx *ctx;
    Solver &S;
    pk_mat *A;
    const pk_comm *comm;
    int steps = 0;
    int overlapped_panels = 0;
    // the exchange of a product's first column panel travels on this stream while the second panel is computed
    hipStream_t side = nullptr;
    hipEvent_t ev_panel = nullptr, ev_summed = nullptr;
    GramianOp(pk_ctx *c, Solver &s, pk_mat *a, const pk_comm *cm) : ctx(c), S(s), A(a), comm(cm) {}
    GramianOp(const GramianOp &) = delete;
    GramianOp &operator=(const GramianOp &) = delete;
    ~GramianOp() {
        if (side) {
            (void)hipStreamSynchronize(side);
            (void)hipStreamDestroy(side);
        }
        if (ev_panel) (void)hipEventDestroy(ev_panel);
        if (ev_summed) (void)hipEventDestroy(ev_summed);
    }
    int allreduce(DMat &M, hipStream_t on = nullptr) {
        if (!comm) return PK_OK;
        if (comm->allreduce_sum_f64(comm->user, M.p(), (int64_t)M.n * M.l, (void *)(on ? on : ctx->stream)) != 0)
            return fail(ctx, PK_E_LAUNCH, "pk_svd_build_sharded: the communicator's all-reduce failed");
        return PK_OK;
    }
    // Is the exchange of an [n_cols x l] block long enough to be worth hiding behind half of its own products?  The rule of
    // solver.py::ItemRows.product (one statement of the solver, two languages): the modelled all-reduce reaches 0.4 ms —
    // the split costs two launches of A^T Y per user block instead of one, and a half-width panel costs ~0.7 of the full
    // launch, not half.  Context option "dist_overlap": 0 = never, 2 = whenever there is something to exchange (tests).
    bool split_product(int l) const {
        if (!comm || comm->world < 2 || l < 32 || l % 16 != 0) return false;
        if (ctx->opt.dist_overlap == 0) return false;
        if (ctx->opt.dist_overlap == 2) return true;
        return 2.0 * (comm->world - 1) / comm->world * (double)A->A.n_cols * l * 8.0 / model::kXgmiBusBps >= 4e-4;
    }
    int ritz(const DMat &X, DMat &H, DMat &Y) {
        Y = DMat(A->A.n_rows, X.l);
        if (!Y.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (Rayleigh-Ritz)");
        CK(spmm_full(ctx, A->A, X, Y));
        CK(S.gram(Y, Y, H));
        return allreduce(H);
    }
    int rotate(const DMat &Y, const DMat &Cm, DMat &Z) {
        DMat Yr;
        CK(S.tsmm(Y, Cm, Yr));
        Z = DMat(A->A.n_cols, Yr.l);
        if (!Z.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (Rayleigh-Ritz)");
        CK(spmm_t(ctx, A, Yr, Z));
        ++steps;
        return allreduce(Z);
    }
    // Z = A^T (A X) with BOTH dense operands gathered from fp32 images (half the bytes per gathered row; fp64 accumulation):
    // a product rounded to ~6e-8 of its norm — for the late steps of a Lanczos build only (solver.py: products='relaxed').
    // One rank, blocks of a multiple of four columns.
    int apply_rounded(const DMat &Xb, DMat &Z) {
        if (comm || Xb.l % 4 != 0) return apply(Xb, Z);
        const int64_t nr = A->A.n_rows, nc = A->A.n_cols;
        const int l = Xb.l;
        Dev X32((size_t)nc * l * 4), Y32((size_t)nr * l * 4);
        DMat Y(nr, l);
        Z = DMat(nc, l);
        if (!X32.p || !Y32.p || !Y.ok() || !Z.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (rounded gramian step)");
        hipLaunchKernelGGL(f64_to_f32_kernel, dim3((unsigned)((nc * l + 255) / 256)), dim3(256), 0, ctx->stream, nc * l, Xb.p(), X32.as<float>());
        CK(spmm(ctx, A->A, X32.p, PK_VAL_F32, l, l, Y.p(), l, Range{0, A->A.plan.n_tasks, 0, A->A.plan.n_long}));
        hipLaunchKernelGGL(f64_to_f32_kernel, dim3((unsigned)((nr * l + 255) / 256)), dim3(256), 0, ctx->stream, nr * l, Y.p(), Y32.as<float>());
        for (int64_t bk = 0; bk < A->n_blocks; ++bk) {
            const int64_t shape3[3] = {bk == 0 ? nc : 0, A->rows_per_block, A->block_nnz[(size_t)bk]};
            CK(spmm(ctx, *A->Tb, Y32.p, PK_VAL_F32, l, l, Z.p(), l, A->block_ranges[(size_t)bk], bk * nc, bk > 0, shape3));
        }
        ++steps;
        return PK_OK;
    }
    int apply(const DMat &Xb, DMat &Z) {
        DMat Y(A->A.n_rows, Xb.l);
        if (!Y.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (gramian step)");
        CK(spmm_full(ctx, A->A, Xb, Y));
        ++steps;
        if (!split_product(Xb.l)) {
            Z = DMat(A->A.n_cols, Xb.l);
            if (!Z.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (gramian step)");
            CK(spmm_t(ctx, A, Y, Z));
            return allreduce(Z);
        }
        // TWO column panels (solver.py::ItemRows.product): the first panel's sum is handed to the communicator on the SIDE
        // stream — the callback's contract is "ordered on the stream it is given": RCCL enqueues there — and the second
        // panel's products are enqueued behind the first's on the context's stream, so they run while that sum travels;
        // the second sum goes on the context's stream, which then waits for the first.  Every rank issues the two sums in
        // the same order.  The panels are contiguous buffers (what a collective wants), joined afterwards.
        if (!side) {
            HIPCK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
            HIPCK(hipEventCreateWithFlags(&ev_panel, hipEventDisableTiming));
            HIPCK(hipEventCreateWithFlags(&ev_summed, hipEventDisableTiming));
        }
        const int w0 = Xb.l / 2, w1 = Xb.l - w0;
        DMat Z0(A->A.n_cols, w0), Z1(A->A.n_cols, w1);
        if (!Z0.ok() || !Z1.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (gramian step panels)");
        // (once the first panel's sum is on the side stream, an error return must not hand Z0 / Z1 back to the pool —
        // which re-issues blocks in the order of the context's stream only — while that collective may still touch Z0)
        auto rest = [&]() -> int {
            CK(spmm_t_cols(ctx, A, Y, 0, w0, Z0));
            HIPCK(hipEventRecord(ev_panel, ctx->stream));
            HIPCK(hipStreamWaitEvent(side, ev_panel, 0));
            CK(allreduce(Z0, side));
            CK(spmm_t_cols(ctx, A, Y, w0, w1, Z1));
            CK(allreduce(Z1));
            HIPCK(hipEventRecord(ev_summed, side));
            HIPCK(hipStreamWaitEvent(ctx->stream, ev_summed, 0));
            CK(S.hcat(&Z0, Z1, Z));
            return PK_OK;
        };
        const int rc = rest();
        if (rc != PK_OK) {
            (void)hipStreamSynchronize(side);
            (void)hipStreamSynchronize(ctx->stream);
            return rc;
        }
        ++overlapped_panels;
        return PK_OK;
    }
};

// a small dense symmetric PSD matrix as the operator: solver.py::_Dense (T X = T^T X is one gram launch)
struct DenseOp {
    pk_ctx *ctx;
    Solver &S;
    const DMat &T;
    int products = 0;
    // T is symmetric: T X is one tall-skinny product over T's rows (ONE launch; the split Gram product + its reduction
    // were two), and a step of the Chebyshev recurrence  Yn = a T Yc + b Yc + c Xc  is that product with an epilogue
    int apply(const DMat &X, DMat &Z) {
        ++products;
        return S.tsmm(T, X, Z);
    }
    int filter_step(const DMat &Yc, double a, double b, double c, const DMat &Xc, DMat &Yn) {
        ++products;
        return S.tsmm_axpby(T, Yc, a, b, &Yc, c, &Xc, Yn);
    }
    int ritz(const DMat &X, DMat &H, DMat &Z) {
        DMat G;
        CK(apply(X, Z));
        CK(S.gram(X, Z, G));
        H = DMat(G.l, G.l);
        if (!H.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (Rayleigh-Ritz)");
        hipLaunchKernelGGL(symmetrize_kernel, dim3((unsigned)((G.l * G.l + 255) / 256)), dim3(256), 0, S.st, G.l, G.p(), H.p());
        return PK_OK;
    }
    int rotate(const DMat &Z, const DMat &Cm, DMat &out) { return S.tsmm(Z, Cm, out); }
};

// ---- the leading pairs of a small dense PSD matrix, with few host reads (round 6) ---------------------------------------
// The filtered subspace iteration above takes a Rayleigh-Ritz step — an l x l eigen-decomposition and four host reads —
// after every filter of the degree the SPREAD of the block allows (degree 4-5 on the projected problems of a Lanczos build:
// theta_1 / theta_l is large), and locks converged pairs with their own projections: ~50 launches and 4-5 reads per outer
// iteration, 3-5 iterations per look — and a look of a narrow-block build costs nine of its steps.  A dense operator this
// small needs neither: the filter is applied in SEGMENTS of the allowed degree with a plain shifted CholeskyQR3 in
// between (no Rayleigh-Ritz, no read, no locking: the block stays l wide), as many segments as the wanted pairs need by the
// Chebyshev amplification of pair k over the damped interval, then ONE Rayleigh-Ritz step.  A warm look whose start pairs
// and their Ritz values are known (the previous look's: a leading principal submatrix keeps them) is one such round: two
// reads.  ok = false hands the problem (and the best orthonormal block) to the subspace iteration: degenerate bounds, a
// Cholesky breakdown, stagnation.
static int dense_topk_segments(pk_ctx *ctx, Solver &S, DenseOp &dop, int k, DMat &X, double tol, const double *lam0, double r0_rel,
                               SubspaceOut &out, bool &ok) {
    ok = false;
    const int l = X.l;
    const int64_t N = X.n;
    const double spread = 1e7, u = 1.1102230246251565e-16;
    const int m_max = 24;
    std::vector<double> lam, res;
    DMat Zr;                         // T X of the current (rotated) block
    auto ritz = [&]() -> int {
        DMat H, Z, Cm, Xr;
        Dev theta_dev;
        CK(dop.ritz(X, H, Z));
        CK(S.eigh(H, lam, Cm, theta_dev));
        CK(S.tsmm(X, Cm, Xr));
        CK(S.tsmm(Z, Cm, Zr));
        CK(S.resid(Zr, Xr, theta_dev, res));
        X = std::move(Xr);
        out.outer += 1;
        return PK_OK;
    };
    auto worst_of = [&]() {
        double w = 0.0;
        const double lam1 = std::max(lam.empty() ? 0.0 : lam[0], 1e-300);
        for (int j = 0; j < k && j < (int)res.size(); ++j) w = std::max(w, res[(size_t)j] / lam1);
        return w;
    };
    double worst = 1e-2;
    bool have_z = false;
    if (lam0) {
        lam.assign(lam0, lam0 + l);
        if (r0_rel >= 0) worst = std::max(r0_rel, tol);
    } else {
        CK(ritz());
        have_z = true;
        worst = worst_of();
        if (worst <= tol) {
            out.lam_all = lam; out.res_act = res; out.n_lock = 0; out.converged = true;
            out.basis = std::move(X);
            ok = true;
            return PK_OK;
        }
    }
    Dev chol_work((size_t)std::max<int64_t>(pk_chol_work_bytes(l), 8)), info(6 * 3 * 4);
    if (!chol_work.p || !info.p) return fail(ctx, PK_E_LAUNCH, "out of device memory (dense_topk_segments)");
    for (int round = 0; round < 10; ++round) {
        const double a0 = lam[0], bnd = lam[(size_t)l - 1];
        const double e = 0.5 * bnd, c = 0.5 * bnd;
        if (!(bnd > 0.0) || !(a0 > c) || k > l) return PK_OK;                    // degenerate spectrum estimate: the general iteration
        const int m = cheb_degree(a0, bnd, spread, m_max);
        const double xk = std::max(2.0 * lam[(size_t)std::min(k, l) - 1] / bnd - 1.0, 1.0 + 1e-9);
        const double amp = std::cosh(m * std::acosh(xk));
        const double need = std::max(worst / tol, 1.0) * 30.0;
        const int nseg = std::max(1, std::min(6, (int)std::ceil(std::log(need) / std::log(std::max(amp, 1.5)))));
        HIPCK(hipMemsetAsync(info.p, 0, 6 * 3 * 4, S.st));
        for (int seg = 0; seg < nseg; ++seg) {
            DMat Z, Yc, Xc;
            if (seg == 0 && have_z) Z = std::move(Zr); else CK(dop.apply(X, Z));
            have_z = false;
            double sigma = e / (a0 - c);
            const double tau = 2.0 / sigma;
            Xc = std::move(X);
            CK(S.axpbypcz(sigma / e, Z, -c * sigma / e, &Xc, 0.0, nullptr, Yc));
            for (int s2 = 2; s2 <= m; ++s2) {
                const double sigma_new = 1.0 / (tau - sigma);
                DMat Yn;
                CK(dop.filter_step(Yc, 2.0 * sigma_new / e, -2.0 * sigma_new * c / e, -sigma * sigma_new, Xc, Yn));
                Xc = std::move(Yc);
                Yc = std::move(Yn);
                sigma = sigma_new;
            }
            // CholeskyQR, verdicts kept on the device.  The first pass factorises the COLUMN-SCALED Gram matrix (pk_chol_rinv_scaled_f64):
            // the columns of a filtered block of Ritz vectors differ by the filter's amplification (up to the spread, 1e7) and are
            // otherwise nearly orthogonal, so the scaled block is well conditioned and ONE shifted pass leaves a block fit for the
            // next filter (between segments); in front of the Rayleigh-Ritz step one plain pass follows (orthonormal to
            // rounding: the scaled pass leaves I + O(shift) = I + 1e-11).  A pass is a 37 us Cholesky plus two small products: the
            // largest item of a look (three unscaled passes per segment: 26.1-26.5 ms per build; two between segments: 24.5;
            // one scaled between segments and two in front of the Rayleigh-Ritz step: 23.2-23.8)
            const int passes = (seg + 1 == nseg) ? 2 : 1;
            for (int p = 0; p < passes; ++p) {
                DMat G, Rinv(l, l), Yn;
                if (!Rinv.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (dense_topk_segments)");
                CK(S.gram(Yc, Yc, G));
                if (p == 0)
                    CK(pk_chol_rinv_scaled_f64(S.st, l, G.p(), l, 11.0 * ((double)N * l + (double)l * (l + 1)) * u, Rinv.p(), l, chol_work.p,
                                               info.as<int32_t>() + 3 * seg + p));
                else
                    CK(pk_chol_rinv_f64(S.st, l, G.p(), l, 0.0, Rinv.p(), l, chol_work.p, info.as<int32_t>() + 3 * seg + p));
                CK(S.tsmm(Yc, Rinv, Yn));
                Yc = std::move(Yn);
            }
            X = std::move(Yc);
        }
        CK(ritz());
        have_z = true;
        int32_t verdicts[18];
        CK(S.to_host(info.p, verdicts, sizeof verdicts));
        bool broke = false;
        for (int32_t v : verdicts) broke = broke || v != 0;
        for (double v : lam) broke = broke || !(v == v);
        if (broke) {
            X = DMat();              // nothing of this block is trusted
            return PK_OK;
        }
        const double now = worst_of();
        if (now <= tol) {
            out.lam_all = lam; out.res_act = res; out.n_lock = 0; out.converged = true;
            out.basis = std::move(X);
            ok = true;
            return PK_OK;
        }
        if (round >= 1 && now > 0.5 * worst) return PK_OK;       // stagnation: the general iteration takes the (orthonormal) block
        worst = now;
    }
    return PK_OK;
}

// the k leading pairs of the dense PSD matrix behind `dop` from the orthonormal start block X: segments first, the
// filtered subspace iteration with locking whenever they hand over
static int dense_topk(pk_ctx *ctx, Solver &S, DenseOp &dop, int k, DMat X, double tol, int max_outer, uint64_t seed, const double *lam0,
                      double r0_rel, SubspaceOut &out, bool cold = false) {
    std::vector<double> lam_cold;
    const int l = X.l;
    const int64_t N = X.n;
    if (cold && l <= 64 && N >= 2 * (int64_t)l) {
        // A COLD solve (no pairs of an earlier look): the l unit vectors span the first blocks of the Krylov space only, and the
        // wanted vectors have weight well beyond them — the segments then spend rounds finding it.  The leading 2l x 2l block of T
        // is a projected matrix in its own right (that of the Krylov space 2l columns in): ONE eigen-decomposition of it
        // (128 x 128: 2.7 ms) gives l start vectors with their Ritz values, from the span of twice as many blocks (fewer
        // products — 57 -> 51 per build — for the same wall time: kept for the Ritz values it hands the first filter).
        const int w = 2 * l;
        DMat Tl(w, w), C2;
        Dev lam_dev;
        if (!Tl.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (dense_topk)");
        HIPCK(hipMemcpy2DAsync(Tl.p(), (size_t)w * 8, dop.T.p(), (size_t)dop.T.l * 8, (size_t)w * 8, (size_t)w, hipMemcpyDeviceToDevice, S.st));
        std::vector<double> lam2;
        CK(S.eigh(Tl, lam2, C2, lam_dev));
        HIPCK(hipMemsetAsync(X.p(), 0, (size_t)N * l * 8, S.st));
        HIPCK(hipMemcpy2DAsync(X.p(), (size_t)l * 8, C2.p(), (size_t)w * 8, (size_t)l * 8, (size_t)w, hipMemcpyDeviceToDevice, S.st));
        lam_cold.assign(lam2.begin(), lam2.begin() + l);
        lam0 = lam_cold.data();
        r0_rel = -1.0;
        out.outer += 1;
    }
    DMat X0;
    CK(S.col_slice(X, 0, X.l, X0));
    bool ok = false;
    // (blocks of at most 64 columns: the Cholesky kernels of wider ones cost more than the Rayleigh-Ritz steps the segments save —
    // rank 100, l = 128: 55.9 -> 65.6 ms per build with three unscaled passes per segment, 44.8 -> 47.5 ms with one scaled pass)
    if (X.l <= 64) CK(dense_topk_segments(ctx, S, dop, k, X, tol, lam0, r0_rel, out, ok));
    if (ok) return PK_OK;
    const int outer0 = out.outer;
    SubspaceOut so;
    CK(subspace_iteration(ctx, S, dop, k, X.ok() && X.l == X0.l ? std::move(X) : std::move(X0), tol, max_outer, 24, 1e7, seed, false, so));
    so.outer += outer0;
    out = std::move(so);
    return PK_OK;
}

// ---- block Lanczos with full reorthogonalisation: solver.py::_block_lanczos restated (synchronous looks: the form the
// Python layer runs with PK_LANCZOS_LAG=0; its side-stream monitors are a host-side scheduling matter) -------------------
struct LanczosOut {
    DMat Vk;                      // [n_items x k]
    std::vector<double> lam_k, res_k;   // Ritz values; TRUE residual norms of the accepted pairs
    int steps = 0, looks = 0, nested_outer = 0, nested_products = 0;
    bool ok = false;              // false: the recurrence broke down or did not converge — the caller runs the subspace iteration
};

// one look: the k leading Ritz pairs of T (N x N) and the residual estimates  sqrt(||T y - th y||^2 + y_last^T S y_last) / th_1
struct RitzLook {
    DMat basis, Yk;
    std::vector<double> lam_all, est;
    Dev lam_k_dev;
    double worst = 0.0;
    bool conv = false;
};

static int ritz_look(pk_ctx *ctx, Solver &S, const DMat &T, const DMat &Sc, const DMat *warm, const std::vector<double> *warm_lam, int k,
                     int b, int width, double est_tol, double prior, uint64_t seed, LanczosOut &lo, RitzLook &out) {
    const int N = (int)T.n;
    DMat X0;
    auto pad = [&](const DMat *src, int l) -> int {
        X0 = DMat(N, l);
        if (!X0.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (ritz_look)");
        if (src) {
            HIPCK(hipMemsetAsync(X0.p(), 0, (size_t)N * l * 8, S.st));
            HIPCK(hipMemcpy2DAsync(X0.p(), (size_t)l * 8, src->p(), (size_t)src->l * 8, (size_t)l * 8, (size_t)src->n, hipMemcpyDeviceToDevice, S.st));
        } else {
            hipLaunchKernelGGL(unit_block_kernel, dim3((unsigned)(((int64_t)N * l + 255) / 256)), dim3(256), 0, S.st, (int64_t)N, l, X0.p());
        }
        return PK_OK;
    };
    CK(pad(warm, warm ? warm->l : std::min(N, std::max(b, width))));      // cold: the first unit vectors, k + guard of them
    double t_in = std::max(0.3 * est_tol, prior < 0 ? 1e-4 : 0.03 * prior);
    bool first_pass = true;
    for (;;) {
        DenseOp dop{ctx, S, T};
        SubspaceOut so;
        // (the start pairs of a warm look keep their Ritz values, and their residual w.r.t. this T is the old coupling estimate)
        const bool warm_pairs = warm && warm_lam && (int)warm_lam->size() == X0.l && prior >= 0;
        CK(dense_topk(ctx, S, dop, k, std::move(X0), t_in, 200, seed, warm_pairs ? warm_lam->data() : nullptr, warm_pairs ? prior : -1.0, so,
                      /*cold=*/!warm && first_pass));
        warm_lam = nullptr;
        first_pass = false;
        lo.nested_outer += so.outer;
        lo.nested_products += dop.products;
        out.basis = std::move(so.basis);
        out.lam_all = so.lam_all;
        out.conv = so.converged;
        CK(S.col_slice(out.basis, 0, k, out.Yk));
        DMat TY;
        CK(S.gram(T, out.Yk, TY));
        if (!out.lam_k_dev.alloc((size_t)k * 8)) return fail(ctx, PK_E_LAUNCH, "out of device memory (ritz_look)");
        CK(S.upload(out.lam_all.data(), out.lam_k_dev.p, (size_t)k * 8));
        std::vector<double> r_in;
        CK(S.resid(TY, out.Yk, out.lam_k_dev, r_in));
        // coupling: y_last^T S y_last per pair, y_last = the last b rows of Yk
        DMat yl(b, k), M(b, k);
        if (!yl.ok() || !M.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (ritz_look)");
        HIPCK(hipMemcpyAsync(yl.p(), out.Yk.p() + (size_t)(N - b) * k, (size_t)b * k * 8, hipMemcpyDeviceToDevice, S.st));
        CK(pk_dgemm_small_f64(S.st, 0, 0, b, k, b, Sc.p(), b, yl.p(), k, M.p(), k));
        std::vector<double> hy((size_t)b * k), hm((size_t)b * k);
        CK(S.to_host(yl.p(), hy.data(), hy.size() * 8));
        CK(S.to_host(M.p(), hm.data(), hm.size() * 8));
        const double lam1 = std::max(out.lam_all.empty() ? 0.0 : out.lam_all[0], 1e-300);
        out.est.assign((size_t)k, 0.0);
        double cmax = 0.0;
        out.worst = 0.0;
        for (int j = 0; j < k; ++j) {
            double c2 = 0.0;
            for (int i = 0; i < b; ++i) c2 += hy[(size_t)i * k + j] * hm[(size_t)i * k + j];
            c2 = std::max(c2, 0.0);
            cmax = std::max(cmax, c2);
            out.est[(size_t)j] = std::sqrt(r_in[(size_t)j] * r_in[(size_t)j] + c2) / lam1;
            out.worst = std::max(out.worst, out.est[(size_t)j]);
        }
        const double coupling = std::sqrt(cmax) / lam1;
        if (t_in <= 0.3 * est_tol || coupling >= 4.0 * t_in || !out.conv) break;
        t_in = std::max(0.3 * est_tol, 0.1 * coupling);
        CK(pad(&out.basis, out.basis.l));
    }
    lo.looks += 1;
    return PK_OK;
}

__global__ void sym_block_kernel(int N, int ld, const double *__restrict__ T, double *__restrict__ out) {   // out[N x N] = (T + T^T) / 2 of a strided T
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * N) return;
    const int r = i / N, c = i - r * N;
    out[i] = 0.5 * (T[(int64_t)r * ld + c] + T[(int64_t)c * ld + r]);
}
// T[rows + c][r] = C[r][c] for r < rows, c < b: the mirror image of a block column of the projected matrix
__global__ void mirror_block_kernel(int rows, int b, int ldt, const double *__restrict__ C, double *__restrict__ T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * b) return;
    const int r = i / b, c = i - r * b;
    T[(int64_t)(rows + c) * ldt + r] = C[i];
}
// Block column j of T from C = Q^T W when W came from a ROUNDED product (W = B Q_j + E_j, |E_j| ~ 6e-8 |W|): only the band is
// kept — T[N-2b .. N) x [N-b, N) and the mirror image of its upper block.  Outside the band C holds Q_i^T E_j: noise that is
// harmless where it stands (it multiplies the small late coefficients of a converging pair) but whose MIRROR image, or the
// symmetrisation of a look, would set it against the O(1) early coefficients — what stalled round 4's rounded products at
// 5e-12.  The exact entries there are zero to rounding under full reorthogonalisation.
__global__ void band_block_kernel(int N, int b, int ldt, const double *__restrict__ C, double *__restrict__ T) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * b) return;
    const int r = i / b, c = i - r * b;
    const bool in_band = r >= N - 2 * b;
    T[(int64_t)r * ldt + (N - b) + c] = in_band ? C[i] : 0.0;
    if (r < N - b) T[(int64_t)(N - b + c) * ldt + r] = in_band ? C[i] : 0.0;
}
struct LanczosBuffers {
    double *Q; int64_t ldq;      // the Krylov basis [n x >= (j + 1) b], block j in columns [(j - 1) b, j b)
    double *T; int64_t ldt;      // the projected matrix [>= j b square]
    double *flags;               // [sum of Cholesky verdicts, max distance of a last pass's Gram matrix from I]
    int32_t *info;               // 3 Cholesky verdicts (scratch)
    void *chol_work;
};

// ONE step of the recurrence (solver.py::_block_lanczos loop body + _next_lanczos_block): W = B Q_j, block column j of T,
// the next block by shifted CholeskyQR3 re-projected against the whole basis in every pass.  Sc = W_perp^T W_perp, the
// coupling behind the residual estimates.  The ONE statement of the step: the coarse build (block_lanczos below) and the
// Python layer's build (pk_lanczos_steps; solver.py keeps the looks, their monitors and the decisions) both run it.
// The step in its two halves: the PRODUCTS  W = A^T (A Q_j)  of the matrix behind `gop` (summed over the ranks inside `gop.apply`
// when the build owns a communicator; a host layer that shards the users itself sums W between the two halves:
// pk_lanczos_products / pk_lanczos_orth), and everything that follows from W on the replicated item side.
static int lanczos_products(pk_ctx *ctx, Solver &S, GramianOp &gop, int64_t n, int b, int j, const LanczosBuffers &B, DMat &W, bool rounded) {
    const int N = j * b;
    DMat Qj(n, b);
    if (!Qj.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (block Lanczos)");
    HIPCK(hipMemcpy2DAsync(Qj.p(), (size_t)b * 8, B.Q + (N - b), (size_t)B.ldq * 8, (size_t)b * 8, (size_t)n, hipMemcpyDeviceToDevice, S.st));
    if (rounded) CK(gop.apply_rounded(Qj, W)); else CK(gop.apply(Qj, W));
    return PK_OK;
}

static int lanczos_orth(pk_ctx *ctx, Solver &S, int64_t n, int b, int j, bool last, const LanczosBuffers &B, const DMat &W, DMat &Sc, bool rounded);

static int lanczos_step(pk_ctx *ctx, Solver &S, GramianOp &gop, int64_t n, int b, int j, bool last, const LanczosBuffers &B, DMat &Sc,
                        bool rounded = false) {
    DMat W;
    CK(lanczos_products(ctx, S, gop, n, b, j, B, W, rounded));
    return lanczos_orth(ctx, S, n, b, j, last, B, W, Sc, rounded);
}

static int lanczos_orth(pk_ctx *ctx, Solver &S, int64_t n, int b, int j, bool last, const LanczosBuffers &B, const DMat &W, DMat &Sc, bool rounded) {
    const int N = j * b;
    const int64_t ldq = B.ldq, ldt = B.ldt;
    const double u = 1.1102230246251565e-16;
    // block column j of T = Q^T W, rows of all blocks so far (and its mirror image)
    DMat C(N, b);
    const size_t need = (size_t)pk_gram_work_bytes(n, N, b);
    if (!C.ok() || (need > S.gram_work.bytes && !S.gram_work.alloc(need))) return fail(ctx, PK_E_LAUNCH, "out of device memory (gram)");
    CK(pk_gram_f64(S.st, n, N, b, B.Q, ldq, W.p(), b, C.p(), b, S.gram_work.p));
    if (rounded && N > 2 * b) {
        hipLaunchKernelGGL(band_block_kernel, dim3((unsigned)(((int64_t)N * b + 255) / 256)), dim3(256), 0, S.st, N, b, (int)ldt, C.p(), B.T);
    } else {
        HIPCK(hipMemcpy2DAsync(B.T + (N - b), (size_t)ldt * 8, C.p(), (size_t)b * 8, (size_t)b * 8, (size_t)N, hipMemcpyDeviceToDevice, S.st));
        if (N > b)
            hipLaunchKernelGGL(mirror_block_kernel, dim3((unsigned)(((int64_t)(N - b) * b + 255) / 256)), dim3(256), 0, S.st, N - b, b, ldt, C.p(),
                               B.T);
    }
    if (!last) {
        // solver.py::_next_lanczos_block: shifted CholeskyQR3, re-projected against the whole basis in every pass
        HIPCK(hipMemsetAsync(B.info, 0, 12, S.st));
        // The block lives where it will stay — columns [N, N + b) of the basis — so that a re-projection pass needs ONE Gram
        // product: [Q | Y]^T Y = (the coefficients Q^T Y of the re-projection; the Gram matrix of Y before it).
        DMat G, M(N + b, b);
        if (!M.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (block Lanczos)");
        const double *Gp = nullptr;
        int64_t ldgp = b;
        for (int p = 0; p < 3; ++p) {
            DMat Yp(n, b), Rinv(b, b);
            if (!Yp.ok() || !Rinv.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (block Lanczos)");
            if (p == 0) {
                CK(pk_tsmm_sub_f64(S.st, n, N, b, B.Q, ldq, C.p(), b, W.p(), b, Yp.p(), b));
                CK(S.gram(Yp, Yp, G));
                CK(S.col_slice(G, 0, b, Sc));
                Gp = G.p();
            } else {
                const size_t need = (size_t)pk_gram_work_bytes(n, N + b, b);
                if (need > S.gram_work.bytes && !S.gram_work.alloc(need)) return fail(ctx, PK_E_LAUNCH, "out of device memory (gram)");
                CK(pk_gram_f64(S.st, n, N + b, b, B.Q, ldq, B.Q + N, ldq, M.p(), b, S.gram_work.p));
                CK(pk_tsmm_sub_f64(S.st, n, N, b, B.Q, ldq, M.p(), b, B.Q + N, ldq, Yp.p(), b));
                Gp = M.p() + (size_t)N * b;
            }
            CK(pk_chol_rinv_f64(S.st, b, Gp, ldgp, p == 0 ? 11.0 * ((double)n * b + (double)b * (b + 1)) * u : 0.0, Rinv.p(), b, B.chol_work,
                                B.info + p));
            CK(pk_tsmm_f64(S.st, n, b, b, Yp.p(), b, Rinv.p(), b, B.Q + N, ldq));
        }
        // flags[0] += the Cholesky verdicts of the three passes; flags[1] = max(flags[1], |G - I|_max) of the last pass's Gram
        // matrix, NaN and inf counted as 1 (the one bookkeeping kernel of the library: dense.hip)
        CK(pk_orth_check_f64(S.st, b, Gp, ldgp, B.info, 3, B.flags));
    } else {
        DMat Wp(n, b);
        if (!Wp.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (block Lanczos)");
        CK(pk_tsmm_sub_f64(S.st, n, N, b, B.Q, ldq, C.p(), b, W.p(), b, Wp.p(), b));
        CK(S.gram(Wp, Wp, Sc));
    }
    return PK_OK;
}

// b: width of a Krylov block; l: width of the nested solves (k + guard vectors).  Round 6: b < l — a narrower block needs
// (l / b)^(0.33 + 0.035 log2(l / b)) times the steps and gathers b / l of the columns per step (solver.py::choose_krylov_block).
// Looks are synchronous here (no side-stream monitors: those are a host-side scheduling matter of solver.py), and a look — a
// nested solve of ~5 ms — costs as much as nine steps of a 16-column block: the first one is taken where the cost model puts
// convergence (a late look wastes cheap steps, an early one costs a whole solve and a second look), later ones where the
// estimate and the measured (or, from one point, the prior) rate put it.
static int block_lanczos(pk_ctx *ctx, Solver &S, GramianOp &gop, int64_t n, int k, int l, int b, double tol, uint64_t seed, int max_steps,
                         double steps_model, LanczosOut &out) {
    // pk_gram_f64 takes operands of at most 4096 columns: a Krylov space that would outgrow them ends the recurrence like
    // any other breakdown (out.ok stays false -> filtered subspace iteration), as solver.py::_block_lanczos does
    int qcap = (int)std::min<int64_t>(n / b, 4096 / b);
    if (qcap < 4 || max_steps < 4) return PK_OK;          // out.ok stays false: no room for a Krylov space
    qcap = std::min(qcap, max_steps);
    int cap = std::min(qcap, 20);
    DMat Q(n, cap * b), T(cap * b, cap * b);
    Dev flags(16), info(12), chol_work((size_t)std::max<int64_t>(pk_chol_work_bytes(b), 8));
    if (!Q.ok() || !T.ok() || !flags.p || !info.p || !chol_work.p) return fail(ctx, PK_E_LAUNCH, "out of device memory (block Lanczos)");
    HIPCK(hipMemsetAsync(T.p(), 0, (size_t)T.n * T.l * 8, S.st));
    HIPCK(hipMemsetAsync(flags.p, 0, 16, S.st));
    {
        DMat R, Q1;
        CK(S.randn(n, b, seed, R));
        CK(S.orthonormalize(R, nullptr, 12345, Q1));
        HIPCK(hipMemcpy2DAsync(Q.p(), (size_t)Q.l * 8, Q1.p(), (size_t)b * 8, (size_t)b * 8, (size_t)n, hipMemcpyDeviceToDevice, S.st));
    }
    std::vector<std::pair<int, double>> hist;
    RitzLook look;
    bool have_warm = false;
    double est_tol = tol;
    int next_look = std::max(std::max(4, (2 * k + b - 1) / b + 2), (l + b - 1) / b);
    if (steps_model > 0) next_look = std::max(next_look, (int)std::ceil(steps_model));
    next_look = std::min(next_look, qcap);
    const double prior_rate = 0.8 * 1.72 * std::pow(b / 16.0, 0.27);      // solver.py::_block_lanczos: natural log per step, late phase
    int j = 0;
    while (j < qcap) {
        ++j;
        const int N = j * b;
        if (std::min(j + 1, qcap) * b > Q.l) {           // grow the basis and the projected matrix (rare: slow convergence)
            const int cap2 = std::min(qcap, std::max(j + 1, (int)(1.5 * cap) + 1));
            DMat Q2(n, cap2 * b), T2(cap2 * b, cap2 * b);
            if (!Q2.ok() || !T2.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (block Lanczos)");
            HIPCK(hipMemsetAsync(T2.p(), 0, (size_t)T2.n * T2.l * 8, S.st));
            HIPCK(hipMemcpy2DAsync(Q2.p(), (size_t)Q2.l * 8, Q.p(), (size_t)Q.l * 8, (size_t)Q.l * 8, (size_t)n, hipMemcpyDeviceToDevice, S.st));
            HIPCK(hipMemcpy2DAsync(T2.p(), (size_t)T2.l * 8, T.p(), (size_t)T.l * 8, (size_t)T.l * 8, (size_t)T.n, hipMemcpyDeviceToDevice, S.st));
            Q = std::move(Q2);
            T = std::move(T2);
            cap = cap2;
        }
        const bool last = j == qcap;
        DMat Sc;
        CK(lanczos_step(ctx, S, gop, n, b, j, last, LanczosBuffers{Q.p(), Q.l, T.p(), T.l, flags.as<double>(), info.as<int32_t>(), chol_work.p}, Sc));
        out.steps = j;
        if (j < next_look && !last) continue;
        // ---- a look: breakdown flags, the pairs of T_j, verification ---------------------------------------------------
        double fl[2];
        CK(S.to_host(flags.p, fl, 16));
        if (fl[0] != 0.0 || !(fl[1] < 1e-4)) return PK_OK;        // the residual block lost rank: out.ok stays false
        DMat Tj(N, N);
        if (!Tj.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (block Lanczos)");
        hipLaunchKernelGGL(sym_block_kernel, dim3((unsigned)(((int64_t)N * N + 255) / 256)), dim3(256), 0, S.st, N, T.l, T.p(), Tj.p());
        RitzLook nl;
        CK(ritz_look(ctx, S, Tj, Sc, have_warm ? &look.basis : nullptr, have_warm ? &look.lam_all : nullptr, k, b, l, est_tol,
                     hist.empty() ? -1.0 : hist.back().second,
                     seed + 1000ull * (uint64_t)j, out, nl));
        look = std::move(nl);
        have_warm = true;
        hist.emplace_back(j, look.worst);
        if (look.worst <= est_tol && look.conv) {
            // one true product on the k Ritz vectors: V = Q Y
            DMat Vk(n, k), Z;
            if (!Vk.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (block Lanczos)");
            CK(pk_tsmm_f64(S.st, n, N, k, Q.p(), Q.l, look.Yk.p(), k, Vk.p(), k));
            CK(gop.apply(Vk, Z));
            std::vector<double> res;
            CK(S.resid(Z, Vk, look.lam_k_dev, res));
            const double lam1 = std::max(look.lam_all[0], 1e-300);
            double worst = 0.0;
            for (double r : res) worst = std::max(worst, r / lam1);
            if (worst <= tol) {
                out.Vk = std::move(Vk);
                out.lam_k.assign(look.lam_all.begin(), look.lam_all.begin() + k);
                out.res_k = res;
                out.ok = true;
                return PK_OK;
            }
            est_tol *= 0.1;
        }
        if (last) break;
        double rate = prior_rate;
        if (hist.size() >= 2 && hist[hist.size() - 2].second > hist.back().second && hist.back().second > 0)
            rate = std::max(0.4, std::log(hist[hist.size() - 2].second / hist.back().second) / (hist.back().first - hist[hist.size() - 2].first));
        const double remaining = std::log(std::max(look.worst, est_tol) / est_tol) / rate;
        next_look = std::min(qcap, j + std::max(1, (int)std::ceil(remaining)));
    }
    return PK_OK;
}

// solver.py::_lanczos_model restated (same constants: polara_amd/machine_model.py)
static void lanczos_model(double nnz, int64_t n_items, int l, int b, int world, double &steps, double &t_step) {
    using namespace model;
    constexpr double kStepFixedS = kLanczosStepFixedS;
    const double ratio = std::max((double)l / b, 1.0);
    steps = (14.0 + std::max(0.0, std::log2(l / 64.0))) * std::pow(ratio, 0.33 + 0.035 * std::log2(ratio));
    double t_spmm = nnz * (8.0 + std::max(b, 16)) * 1e-12 / world;
    if (world > 1) t_spmm += 2.0 * (world - 1) / world * (double)n_items * b * 8.0 / kXgmiBusBps + 6 * (world - 1) * kCollectiveStepS;
    const double n_avg = 0.5 * steps * b;
    t_step = t_spmm + kStepFixedS + 14.0 * (double)n_items * n_avg * b / kDenseF64Flops / world;
}

static int svd_build_impl(pk_ctx *ctx, pk_mat *A, const pk_comm *comm, int32_t k, int32_t block, double tol, int32_t max_outer,
                          uint64_t seed, double *sigma_out, double *V_out, double *U_out, pk_build_stats *stats_out) {
    if (!ctx || !A) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    (void)hipSetDevice(ctx->device);
    const int64_t n_items = A->A.n_cols, n_users = A->A.n_rows;
    if (k < 1 || k > n_items || !sigma_out || !V_out) return fail(ctx, PK_E_INVALID, "pk_svd_build: k must satisfy 0 < k <= n_items; outputs required");
    if (tol <= 0) tol = 1e-12;
    if (max_outer <= 0) max_outer = 200;
    const int m_max = 24;
    const double spread = 1e7;
    int l = block;
    if (l <= 0) {
        const int over = std::max(14, (28 * k + 99) / 100);
        l = ((k + over + 7) / 8) * 8;
    }
    l = (int)std::max<int64_t>(k, std::min<int64_t>(l, n_items));
    if (l > 1024) return fail(ctx, PK_E_UNSUPPORTED, "pk_svd_build: block width %d beyond the 1024 of the dense kernels", l);
    Solver S{ctx, ctx->stream, Dev()};
    pk_build_stats stats;
    memset(&stats, 0, sizeof(stats));
    stats.block = l;

    DMat X;
    {
        DMat R;
        CK(S.randn(n_items, l, seed, R));
        CK(S.orthonormalize(R, nullptr, 12345, X));
    }
    GramianOp gop{ctx, S, A, comm};
    // the method, as solver.py::svd_topk chooses it: block Lanczos where a Gramian step is heavy (stored entries x block
    // width, summed over the ranks), the filtered subspace iteration on small matrices and whenever the Krylov recurrence
    // breaks down (context option "svd_method" overrides)
    bool use_lanczos;
    int kb = l;
    double work_total = 0.0;
    const int world_size = comm ? comm->world : 1;
    {
        double work = (double)A->A.nnz;
        if (comm) {
            Dev wd(8);
            if (!wd.p) return fail(ctx, PK_E_LAUNCH, "out of device memory");
            CK(S.upload(&work, wd.p, 8));
            if (comm->allreduce_sum_f64(comm->user, wd.p, 1, (void *)ctx->stream) != 0)
                return fail(ctx, PK_E_LAUNCH, "pk_svd_build_sharded: the communicator's all-reduce failed");
            CK(S.to_host(wd.p, &work, 8));
        }
        // solver.py::choose_method / choose_krylov_block / _lanczos_model, restated with the same constants
        // (polara_amd/machine_model.py — measured rates with their records under profiles/, and the two multi-GPU figures
        // that are assumptions because no N > 1 run exists)
        work_total = work;
        const int world = world_size;
        auto model = [&](int b, double &steps, double &t_step) { lanczos_model(work, n_items, l, b, world, steps, t_step); };
        static const int widths[] = {16, 32, 64, 128, 256};
        double best_t = -1.0;
        for (int w : widths) {
            if (w > l && best_t >= 0) break;
            const int b = std::min(w, l);
            double steps, t_step;
            model(b, steps, t_step);
            if (best_t < 0 || steps * t_step < best_t) { best_t = steps * t_step; kb = b; }
        }
        constexpr double kNestedSolveS = model::kNestedSolveS, kStepFixedS = model::kLanczosStepFixedS;
        const double wide2 = std::max(1.0, (l / 64.0) * (l / 64.0));
        double steps_l, t_wide;
        model(l, steps_l, t_wide);
        const double t_lanczos = best_t + 4.0 * kNestedSolveS * wide2;
        const double t_subspace = 2.6 * 14.0 * (t_wide - kStepFixedS) + 8 * 0.5e-3 * wide2;
        use_lanczos = ctx->opt.svd_method == 1 ? true : ctx->opt.svd_method == 2 ? false : t_lanczos < t_subspace;
        if (ctx->opt.krylov_block > 0) kb = std::max(1, std::min(ctx->opt.krylov_block, l));
    }
    CK(ensure_blocked_transpose(ctx, A, use_lanczos ? kb : l));
    DMat Vk;
    std::vector<double> lam_k, res_host;
    int n_lock = 0;
    bool have = false;
    if (use_lanczos) {
        LanczosOut lo;
        const int max_steps = std::min(4096 / kb, (int)(64.0 * std::sqrt((double)l / kb)));
        double steps_model, t_step_model;
        lanczos_model(work_total, n_items, l, kb, world_size, steps_model, t_step_model);
        CK(block_lanczos(ctx, S, gop, n_items, k, l, kb, tol, seed, std::min(max_steps, 4 * max_outer), steps_model, lo));
        stats.outer = lo.looks;
        if (lo.ok) {
            Vk = std::move(lo.Vk);
            lam_k = lo.lam_k;
            res_host = lo.res_k;
            stats.converged = 1;
            have = true;
        }
    }
    if (!have) {
        SubspaceOut so;
        CK(subspace_iteration(ctx, S, gop, k, std::move(X), tol, max_outer, m_max, spread, seed, true, so));
        stats.outer = so.outer;
        stats.converged = so.converged ? 1 : 0;
        n_lock = so.n_lock;
        res_host = so.res_act;
        const int take = std::min<int>(k, so.basis.l);
        CK(S.col_slice(so.basis, 0, take, Vk));
        lam_k.assign(so.lam_all.begin(), so.lam_all.begin() + std::min<size_t>((size_t)k, so.lam_all.size()));
    }
    stats.gramian_steps = gop.steps;
    const int kk = std::min<int>(k, Vk.l);
    // to the host: sigma descending, V column-major (the F-ordered `vh.T` of models.py:849)
    std::vector<double> vh((size_t)n_items * Vk.l);
    CK(S.to_host(Vk.p(), vh.data(), vh.size() * 8));
    std::vector<int> order((size_t)kk);
    std::iota(order.begin(), order.end(), 0);
    for (auto &v : lam_k) v = std::max(v, 0.0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b2) { return lam_k[(size_t)a] > lam_k[(size_t)b2]; });
    for (int j = 0; j < kk; ++j) {
        sigma_out[j] = std::sqrt(lam_k[(size_t)order[(size_t)j]]);
        for (int64_t i = 0; i < n_items; ++i) V_out[(size_t)j * n_items + i] = vh[(size_t)i * Vk.l + order[(size_t)j]];
    }
    for (int j = kk; j < k; ++j) sigma_out[j] = 0.0;
    double worst = 0.0;
    if (!res_host.empty()) {
        const int cnt = std::max(1, std::min<int>(k - n_lock, (int)res_host.size()));
        for (int j = 0; j < cnt; ++j) worst = std::max(worst, res_host[(size_t)j]);
    }
    stats.final_rel_residual = worst / std::max(lam_k.empty() ? 1.0 : *std::max_element(lam_k.begin(), lam_k.end()), 1e-300);
    if (U_out) {
        // U = A V Sigma^-1, column-major [n_users x k]
        DMat Vs(n_items, kk), U(n_users, kk);
        if (!Vs.ok() || !U.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (user factors)");
        std::vector<double> vr((size_t)n_items * kk);
        for (int j = 0; j < kk; ++j)
            for (int64_t i = 0; i < n_items; ++i) vr[(size_t)i * kk + j] = V_out[(size_t)j * n_items + i];
        CK(S.upload(vr.data(), Vs.p(), vr.size() * 8));
        CK(spmm_full(ctx, A->A, Vs, U));
        std::vector<double> uh((size_t)n_users * kk);
        CK(S.to_host(U.p(), uh.data(), uh.size() * 8));
        for (int j = 0; j < kk; ++j) {
            const double inv = sigma_out[j] > 0 ? 1.0 / sigma_out[j] : 0.0;
            for (int64_t i = 0; i < n_users; ++i) U_out[(size_t)j * n_users + i] = uh[(size_t)i * kk + j] * inv;
        }
    }
    if (stats_out) *stats_out = stats;
    if (!stats.converged) {
        fail(ctx, PK_E_NOCONV, "pk_svd_build: not converged in %d outer iterations (worst relative residual %.3e, tolerance %.1e); "
                               "the best available factors were written", stats.outer, stats.final_rel_residual, tol);
        return PK_E_NOCONV;
    }
    return PK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// The recurrence of the block Lanczos build for a host layer that keeps the looks (polara_amd/solver.py::_block_lanczos:
// monitors on a side stream, the schedule of looks, the verification): a NON-OWNING matrix over CSR arrays that already live
// in HBM, steps of the recurrence on buffers of the caller, and the Gramian product for the verification — all on the stream
// the caller names, temporaries from the context's pool.
// ------------------------------------------------------------------------------------------------------------
struct StreamScope {        // the context's stream is the caller's for the duration of one call (the context mutex is held)
    pk_ctx *ctx;
    hipStream_t prev;
    StreamScope(pk_ctx *c, void *stream) : ctx(c), prev(c->stream) { c->stream = pk_stream(stream); }      // (0 = the null stream, where torch's default stream lives)
    ~StreamScope() { ctx->stream = prev; }
};

extern "C" int pk_mat_wrap_device(pk_ctx *ctx, void *stream, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *indptr_dev,
                                  const int32_t *indices_dev, const void *values_dev, int32_t val_kind, int32_t block_cols,
                                  pk_mat **out) {
    if (!ctx || !out) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    StreamScope stream_scope(ctx, stream);
    (void)hipSetDevice(ctx->device);
    if (n_rows < 1 || n_cols < 1 || nnz < 0 || !indptr_dev || (nnz && (!indices_dev || !values_dev)) ||
        (val_kind != PK_VAL_F32 && val_kind != PK_VAL_F64))
        return fail(ctx, PK_E_INVALID, "pk_mat_wrap_device: bad arguments");
    auto m = std::make_unique<pk_mat>();
    Csr &A = m->A;
    A.n_rows = n_rows; A.n_cols = n_cols; A.nnz = nnz; A.val_kind = val_kind;
    A.indptr.borrow(indptr_dev, (size_t)(n_rows + 1) * 8);
    A.indices.borrow(indices_dev, (size_t)nnz * 4);
    A.values.borrow(values_dev, (size_t)nnz * (val_kind == PK_VAL_F32 ? 4 : 8));
    m->nonneg = false;          // not examined: the wrapped matrix serves products only
    int rc = build_plan(ctx, A);
    if (rc != PK_OK) return rc;
    rc = ensure_blocked_transpose(ctx, m.get(), block_cols > 0 ? block_cols : 64);
    if (rc != PK_OK) return rc;
    *out = m.release();
    return PK_OK;
}

extern "C" int pk_lanczos_steps(pk_ctx *ctx, void *stream, pk_mat *A, int32_t b, int32_t j0, int32_t m, int32_t last_closes,
                                double *Q_dev, int64_t ldq, double *T_dev, int64_t ldt, double *S_out_dev, double *flags_dev,
                                int32_t rounded) {
    if (!ctx || !A) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    StreamScope stream_scope(ctx, stream);
    (void)hipSetDevice(ctx->device);
    const int64_t n = A->A.n_cols;
    if (b < 1 || b > 1024 || j0 < 0 || m < 1 || !Q_dev || !T_dev || !S_out_dev || !flags_dev || !A->Tb ||
        ldq < (int64_t)(j0 + m + (last_closes ? 0 : 1)) * b || ldt < (int64_t)(j0 + m) * b || (int64_t)(j0 + m) * b > 4096)
        return fail(ctx, PK_E_INVALID, "pk_lanczos_steps: bad arguments (b=%d, j0=%d, m=%d)", b, j0, m);
    Solver S{ctx, ctx->stream, Dev()};
    GramianOp gop{ctx, S, A, nullptr};
    Dev info(12), chol_work((size_t)std::max<int64_t>(pk_chol_work_bytes(b), 8));
    if (!info.p || !chol_work.p) return fail(ctx, PK_E_LAUNCH, "out of device memory (pk_lanczos_steps)");
    for (int j = j0 + 1; j <= j0 + m; ++j) {
        DMat Sc;
        CK(lanczos_step(ctx, S, gop, n, b, j, last_closes && j == j0 + m, LanczosBuffers{Q_dev, ldq, T_dev, ldt, flags_dev, info.as<int32_t>(), chol_work.p}, Sc,
                        rounded != 0));
        if (j == j0 + m) HIPCK(hipMemcpyAsync(S_out_dev, Sc.p(), (size_t)b * b * 8, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return PK_OK;
}

// The two halves of a step for a host layer that shards the USERS itself (one process per GPU, item side replicated): every
// rank computes the products of ITS rows, the host sums W over the ranks (one all-reduce of n_items x b per step — RCCL), every
// rank runs the same orthogonalisation on the same sum.  polara_amd/solver.py::_block_lanczos on more than one rank.
extern "C" int pk_lanczos_products(pk_ctx *ctx, void *stream, pk_mat *A, int32_t b, int32_t j, const double *Q_dev, int64_t ldq,
                                   double *W_out_dev, int32_t rounded) {
    if (!ctx || !A) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    StreamScope stream_scope(ctx, stream);
    (void)hipSetDevice(ctx->device);
    const int64_t n = A->A.n_cols;
    if (b < 1 || b > 1024 || j < 1 || !Q_dev || !W_out_dev || !A->Tb || ldq < (int64_t)j * b)
        return fail(ctx, PK_E_INVALID, "pk_lanczos_products: bad arguments (b=%d, j=%d)", b, j);
    Solver S{ctx, ctx->stream, Dev()};
    GramianOp gop{ctx, S, A, nullptr};
    DMat W;
    CK(lanczos_products(ctx, S, gop, n, b, j, LanczosBuffers{const_cast<double *>(Q_dev), ldq, nullptr, 0, nullptr, nullptr, nullptr}, W, rounded != 0));
    HIPCK(hipMemcpyAsync(W_out_dev, W.p(), (size_t)n * b * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return PK_OK;
}

extern "C" int pk_lanczos_orth(pk_ctx *ctx, void *stream, int64_t n_items, int32_t b, int32_t j, int32_t last_closes, double *Q_dev,
                               int64_t ldq, double *T_dev, int64_t ldt, const double *W_dev, double *S_out_dev, double *flags_dev,
                               int32_t rounded) {
    if (!ctx) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    StreamScope stream_scope(ctx, stream);
    (void)hipSetDevice(ctx->device);
    if (n_items < 1 || b < 1 || b > 1024 || j < 1 || !Q_dev || !T_dev || !W_dev || !S_out_dev || !flags_dev ||
        ldq < (int64_t)(j + (last_closes ? 0 : 1)) * b || ldt < (int64_t)j * b || (int64_t)j * b > 4096)
        return fail(ctx, PK_E_INVALID, "pk_lanczos_orth: bad arguments (b=%d, j=%d)", b, j);
    Solver S{ctx, ctx->stream, Dev()};
    Dev info(12), chol_work((size_t)std::max<int64_t>(pk_chol_work_bytes(b), 8));
    if (!info.p || !chol_work.p) return fail(ctx, PK_E_LAUNCH, "out of device memory (pk_lanczos_orth)");
    DMat W = DMat::view(W_dev, n_items, b), Sc;
    CK(lanczos_orth(ctx, S, n_items, b, j, last_closes != 0, LanczosBuffers{Q_dev, ldq, T_dev, ldt, flags_dev, info.as<int32_t>(), chol_work.p}, W, Sc,
                    rounded != 0));
    HIPCK(hipMemcpyAsync(S_out_dev, Sc.p(), (size_t)b * b * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return PK_OK;
}

extern "C" int pk_gramian_apply_f64(pk_ctx *ctx, void *stream, pk_mat *A, int32_t nc, const double *X_dev, int64_t ldx, double *Z_dev,
                                    int64_t ldz) {
    if (!ctx || !A) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    StreamScope stream_scope(ctx, stream);
    (void)hipSetDevice(ctx->device);
    if (nc < 1 || nc > 1024 || !X_dev || !Z_dev || ldx < nc || ldz < nc || !A->Tb)
        return fail(ctx, PK_E_INVALID, "pk_gramian_apply_f64: bad arguments (nc=%d)", nc);
    const int64_t n = A->A.n_cols;
    Solver S{ctx, ctx->stream, Dev()};
    GramianOp gop{ctx, S, A, nullptr};
    DMat X(n, nc), Z;
    if (!X.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (pk_gramian_apply_f64)");
    HIPCK(hipMemcpy2DAsync(X.p(), (size_t)nc * 8, X_dev, (size_t)ldx * 8, (size_t)nc * 8, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    CK(gop.apply(X, Z));
    HIPCK(hipMemcpy2DAsync(Z_dev, (size_t)ldz * 8, Z.p(), (size_t)nc * 8, (size_t)nc * 8, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    return PK_OK;
}

// The fp32 image of the item factors the approximate fold-in gathers from (polara_amd/scoring.py::FactorImage; the serving
// handle below builds the same): out [n x ld32] = fl32(V) in columns 0..K-1, the row-norm bound in column K, zeros beyond;
// stat_dev[0] = the bits of the largest bound (non-negative floats order like their bits), stat_dev[1] != 0 when an entry
// of V or a bound is not finite — the two numbers FactorImage's range check needs, in the same launch.
__global__ void v32_image_stat_kernel(int64_t n, int K, int ld32, const double *__restrict__ V, int64_t ldv, const float *__restrict__ bound,
                                      float *__restrict__ out, uint32_t *__restrict__ stat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * ld32) return;
    const int64_t r = i / ld32;
    const int c = (int)(i - r * ld32);
    float v = 0.0f;
    if (c < K) {
        const double d = V[r * ldv + c];
        v = (float)d;
        if (!(fabs(d) <= 1.7976931348623157e308)) atomicOr(&stat[1], 1u);
    } else if (c == K) {
        v = bound[r];
        if (!(v >= 0.0f && v <= 3.4028234e38f)) atomicOr(&stat[1], 1u); else atomicMax(&stat[0], __float_as_uint(v));
    }
    out[i] = v;
}

extern "C" int pk_v32_image_f32(void *stream, int64_t n, int32_t K, int32_t ld32, const double *V_dev, int64_t ldv, const float *bound_dev,
                                float *out_dev, uint32_t *stat_dev) {
    PK_REQUIRE(n >= 0 && K >= 1 && ld32 > K && ldv >= K && V_dev && bound_dev && out_dev && stat_dev, "pk_v32_image_f32: bad arguments");
    hipStream_t st = pk_stream(stream);
    (void)hipMemsetAsync(stat_dev, 0, 8, st);
    if (n > 0)
        hipLaunchKernelGGL(v32_image_stat_kernel, dim3((unsigned)(((size_t)n * ld32 + 255) / 256)), dim3(256), 0, st, n, K, ld32, V_dev, ldv, bound_dev,
                           out_dev, stat_dev);
    PK_CHECK_LAUNCH("v32_image_stat_kernel");
    return PK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// pk_sym_eig_topk_f64: the k leading eigenpairs of a small dense symmetric PSD matrix that lives on the device — the
// projected problem T = Q^T (A^T A) Q of the block Lanczos build (solver.py::_block_lanczos; the reference's svds solves
// the same projected problem inside ARPACK, models.py:844).  It is the filtered subspace iteration above with T as the
// operator, run from C++: a nested solve is a few hundred launches of kernels that take microseconds, and from Python
// every one of them costs the host ~20 us — 20 of the 48 ms of the first Lanczos build.
// ------------------------------------------------------------------------------------------------------------
extern "C" int pk_sym_eig_topk_f64(pk_ctx *ctx, void *stream, int32_t n, const double *T_dev, int64_t ldt, int32_t k, int32_t l,
                                   const double *X0_dev, int64_t ldx0, int32_t x0_rows, double tol, int32_t max_outer, uint64_t seed,
                                   double *basis_out_dev, int64_t ldb, double *lam_out_host, double *res_out_host,
                                   int32_t *counts_out, const double *lam0_host, double r0_rel) {
    if (!ctx) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    (void)hipSetDevice(ctx->device);
    if (n < 1 || k < 1 || l < k || l > n || l > 1024 || !T_dev || ldt < n || !basis_out_dev || ldb < l || !lam_out_host || !res_out_host ||
        !counts_out || (X0_dev && (x0_rows < 1 || x0_rows > n || ldx0 < l)))
        return fail(ctx, PK_E_INVALID, "pk_sym_eig_topk_f64: bad arguments (n=%d, k=%d, l=%d)", n, k, l);
    if (tol <= 0) tol = 1e-13;
    if (max_outer <= 0) max_outer = 200;
    hipStream_t st = stream ? pk_stream(stream) : ctx->stream;
    Solver S{ctx, st, Dev()};
    DMat T(n, n), X(n, l);
    if (!T.ok() || !X.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (pk_sym_eig_topk_f64)");
    HIPCK(hipMemcpy2DAsync(T.p(), (size_t)n * 8, T_dev, (size_t)ldt * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToDevice, st));
    if (X0_dev) {
        HIPCK(hipMemsetAsync(X.p(), 0, (size_t)n * l * 8, st));
        HIPCK(hipMemcpy2DAsync(X.p(), (size_t)l * 8, X0_dev, (size_t)ldx0 * 8, (size_t)l * 8, (size_t)x0_rows, hipMemcpyDeviceToDevice, st));
    } else {
        hipLaunchKernelGGL(unit_block_kernel, dim3((unsigned)(((int64_t)n * l + 255) / 256)), dim3(256), 0, st, (int64_t)n, l, X.p());
    }
    DenseOp dop{ctx, S, T};
    SubspaceOut so;
    CK(dense_topk(ctx, S, dop, k, std::move(X), tol, max_outer, seed, X0_dev ? lam0_host : nullptr, r0_rel, so, /*cold=*/X0_dev == nullptr));
    const int w = std::min<int>(l, so.basis.l);
    HIPCK(hipMemcpy2DAsync(basis_out_dev, (size_t)ldb * 8, so.basis.p(), (size_t)so.basis.l * 8, (size_t)w * 8, (size_t)n,
                           hipMemcpyDeviceToDevice, st));
    HIPCK(hipStreamSynchronize(st));
    for (int j = 0; j < l; ++j) lam_out_host[j] = j < (int)so.lam_all.size() ? so.lam_all[(size_t)j] : 0.0;
    for (int j = 0; j < l; ++j) res_out_host[j] = j < (int)so.res_act.size() ? so.res_act[(size_t)j] : 0.0;
    counts_out[0] = so.n_lock;
    counts_out[1] = w - so.n_lock;
    counts_out[2] = so.converged ? 1 : 0;
    counts_out[3] = so.outer;
    counts_out[4] = dop.products;
    return PK_OK;
}

// ------------------------------------------------------------------------------------------------------------
// pk_serving_* / pk_score_topk: polara_amd/scoring.py::recommend restated (models.py:391-405, 857-861, 494-519, 488-491)
// A serving handle keeps what a model keeps between get_recommendations() calls: the item factors in the serving
// order (descending factor norm) with their images, and the test matrix renamed into that order with its task plan and
// seen-tile streams.  pk_score_topk = create + score + free.
// ------------------------------------------------------------------------------------------------------------
struct pk_serving {
    int64_t n_items = 0, n_users = 0;
    int K = 0, ld32 = 0, Kx_full = 0;
    double vmax = 0.0;
    bool nonneg = true, have_tiles = false, have_v32 = false, fused = false;
    Dev inv64;                 // serving position -> the caller's item id (int64, for pk_map_ids_i64)
    DMat V;
    Csr Ts;
    Dev Vp, tile_bound, V32, tiles, ntiles, dense, skip;
    Dev vnorm, q20_raw, q20_tab;     // fp32 norm bounds of the item rows; the packed fold-in image (csrc/foldq.hip) and its bracket scales
    char *q20_img = nullptr;      // 128-byte aligned start of the image inside q20_raw (nullptr: no packed image)
    int dense_tiles = 0;          // window of the dense seen masks (0: none)
    Dev exact_work;               // row slots + tickets of the exact-row tail (rescore.hip: pk_exact_work_bytes), tickets zeroed once
};

namespace {

int serving_build(pk_ctx *ctx, pk_serving *sv, int64_t n_items, int32_t K, const double *V_host, pk_mat *T) {
    hipStream_t st = ctx->stream;
    const int64_t n_users = T->A.n_rows;
    Solver S{ctx, st, Dev()};
    sv->n_items = n_items; sv->n_users = n_users; sv->K = K; sv->nonneg = T->nonneg; sv->fused = K <= 256;
    // serving order: items by descending factor norm (the pruning bound is a suffix maximum of these norms)
    std::vector<double> norm((size_t)n_items, 0.0);
    for (int j = 0; j < K; ++j)
        for (int64_t i = 0; i < n_items; ++i) { const double v = V_host[(size_t)j * n_items + i]; norm[(size_t)i] += v * v; }
    double vmax = 0.0;
    for (auto &v : norm) { v = std::sqrt(v); vmax = std::max(vmax, v); }
    if (!std::isfinite(vmax) || (vmax != 0.0 && !(vmax > 1e-30 && vmax < 1e30)))
        return fail(ctx, PK_E_INVALID, "pk_score_topk: item factors with max row norm %g are outside the fp32 range of the candidate sweep", vmax);
    sv->vmax = vmax;
    std::vector<int32_t> inv((size_t)n_items), rank_of((size_t)n_items);
    std::iota(inv.begin(), inv.end(), 0);
    std::stable_sort(inv.begin(), inv.end(), [&](int32_t a, int32_t b) { return norm[(size_t)a] > norm[(size_t)b]; });
    for (int64_t i = 0; i < n_items; ++i) rank_of[(size_t)inv[(size_t)i]] = (int32_t)i;
    {
        std::vector<int64_t> inv_l(inv.begin(), inv.end());
        if (!sv->inv64.alloc((size_t)n_items * 8)) return fail(ctx, PK_E_LAUNCH, "out of device memory (item ids)");
        CK(S.upload(inv_l.data(), sv->inv64.p, (size_t)n_items * 8));
    }
    std::vector<double> vr((size_t)n_items * K);
    for (int64_t i = 0; i < n_items; ++i)
        for (int j = 0; j < K; ++j) vr[(size_t)i * K + j] = V_host[(size_t)j * n_items + inv[(size_t)i]];
    sv->V = DMat(n_items, K);
    DMat &V = sv->V;
    if (!V.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (factors)");
    CK(S.upload(vr.data(), V.p(), vr.size() * 8));
    // the test rows in the serving order (rows re-sorted: canonical CSR)
    Csr &Ts = sv->Ts;
    Ts.n_rows = n_users; Ts.n_cols = n_items; Ts.nnz = T->A.nnz; Ts.val_kind = T->A.val_kind;
    const size_t ve = Ts.val_kind == PK_VAL_F32 ? 4 : 8, n1 = (size_t)std::max<int64_t>(Ts.nnz, 1);
    {
        Dev cmap((size_t)n_items * 4), work((size_t)pk_csr_relabel_work_bytes(Ts.nnz));
        if (!cmap.p || !work.p || !Ts.indptr.alloc((size_t)(n_users + 1) * 8) || !Ts.indices.alloc(n1 * 4) || !Ts.values.alloc(n1 * ve))
            return fail(ctx, PK_E_LAUNCH, "out of device memory (test matrix)");
        CK(S.upload(rank_of.data(), cmap.p, (size_t)n_items * 4));
        HIPCK(hipMemcpyAsync(Ts.indptr.p, T->A.indptr.p, (size_t)(n_users + 1) * 8, hipMemcpyDeviceToDevice, st));
        CK(pk_csr_relabel_sorted(st, n_users, n_items, Ts.nnz, T->A.indptr.as<int64_t>(), T->A.indices.as<int32_t>(), T->A.values.p,
                                 Ts.val_kind, cmap.as<int32_t>(), Ts.indices.as<int32_t>(), Ts.values.p, work.p));
        HIPCK(hipStreamSynchronize(st));
    }
    CK(build_plan(ctx, Ts));
    if (!sv->fused) return PK_OK;
    // factor images: MFMA fragments, tile bounds, fp32 image with the norm column
    Dev tb_work((size_t)n_items * 4), rowb((size_t)n_items * 4);
    if (!sv->Vp.alloc((size_t)pk_pack_elems(n_items, K) * 4) || !sv->tile_bound.alloc((size_t)((n_items + 31) / 32) * 4) || !tb_work.p || !rowb.p)
        return fail(ctx, PK_E_LAUNCH, "out of device memory (factor images)");
    CK(pk_pack_frag_f32(st, n_items, K, V.p(), K, sv->Vp.as<float>()));
    CK(pk_tile_norm_bound_f32(st, n_items, K, V.p(), K, tb_work.as<float>(), sv->tile_bound.as<float>()));
    sv->Kx_full = ((K + 1 + 3) / 4) * 4;
    sv->ld32 = sv->Kx_full > 16 ? ((sv->Kx_full + 31) / 32) * 32 : (sv->Kx_full <= 4 ? 4 : sv->Kx_full <= 8 ? 8 : 16);
    if (sv->Kx_full <= 256 && sv->nonneg) {
        if (!sv->V32.alloc((size_t)n_items * sv->ld32 * 4)) return fail(ctx, PK_E_LAUNCH, "out of device memory (fp32 image)");
        CK(pk_row_norm_bound_f32(st, n_items, K, V.p(), K, rowb.as<float>()));
        hipLaunchKernelGGL(v32_image_kernel, dim3((unsigned)(((size_t)n_items * sv->ld32 + 255) / 256)), dim3(256), 0, st, n_items, K, sv->ld32,
                           V.p(), rowb.as<float>(), sv->V32.as<float>());
        sv->have_v32 = true;
        // the items' own norm bounds for the certification (scoring.py: FactorImage.vnorm) ...
        if (!sv->vnorm.alloc((size_t)n_items * 4)) return fail(ctx, PK_E_LAUNCH, "out of device memory (item norms)");
        HIPCK(hipMemcpyAsync(sv->vnorm.p, rowb.p, (size_t)n_items * 4, hipMemcpyDeviceToDevice, st));
        // ... and the packed image of the approximate fold-in (FactorImage.Q20): one cache line per rank-50 row
        const int64_t qbytes = pk_q20_image_bytes(n_items, K);
        if (qbytes > 0 && n_items < (1 << 24) && qbytes < ((int64_t)1 << 32)) {
            Dev qwork(768), qinfo(4);
            if (!sv->q20_raw.alloc((size_t)qbytes + 128) || !sv->q20_tab.alloc(96 * 8) || !qwork.p || !qinfo.p)
                return fail(ctx, PK_E_LAUNCH, "out of device memory (packed image)");
            char *img = static_cast<char *>(sv->q20_raw.p);
            img += (128 - (reinterpret_cast<uintptr_t>(img) & 127)) & 127;
            CK(pk_q20_encode_f64(st, n_items, K, V.p(), K, img, sv->q20_tab.as<double>(), qwork.p, qinfo.as<int32_t>()));
            int32_t info = 0;
            CK(S.to_host(qinfo.p, &info, 4));
            if (info == 0) sv->q20_img = img;      // (else: factors outside the format's range — the fp32 image serves)
        }
    }
    HIPCK(hipStreamSynchronize(st));   // tb_work / rowb go back to the pool
    return PK_OK;
}

int serving_score(pk_ctx *ctx, pk_serving *sv, int32_t topk, int32_t filter_seen, int64_t *out_idx, double *out_scores) {
    hipStream_t st = ctx->stream;
    const int64_t n_items = sv->n_items, n_users = sv->n_users;
    const int K = sv->K;
    if (!out_idx || topk < 1) return fail(ctx, PK_E_INVALID, "pk_score_topk: bad arguments");
    if (topk > n_items) return fail(ctx, PK_E_INVALID, "kth(=%lld) out of bounds (%lld)", (long long)(n_items - topk), (long long)n_items);
    Solver S{ctx, st, Dev()};
    DMat &V = sv->V;
    Csr &Ts = sv->Ts;
    const double vmax = sv->vmax;
    const size_t n1 = (size_t)std::max<int64_t>(Ts.nnz, 1);
    const Range all{0, Ts.plan.n_tasks, 0, Ts.plan.n_long};
    const int64_t *seen_ptr = filter_seen ? Ts.indptr.as<int64_t>() : nullptr;
    const int32_t *seen_idx = filter_seen ? Ts.indices.as<int32_t>() : nullptr;
    Dev out_i((size_t)n_users * topk * 8), out_s((size_t)n_users * topk * 8), flags((size_t)n_users * 4), lst((size_t)std::max<int64_t>(n_users, 1) * 4), cnt(4);
    Dev lst2((size_t)std::max<int64_t>(n_users, 1) * 4), cnt2(8);
    if (!out_i.p || !out_s.p || !flags.p || !lst.p || !cnt.p || !lst2.p || !cnt2.p) return fail(ctx, PK_E_LAUNCH, "out of device memory (outputs)");
    const int KC = sv->fused ? pk_candidate_capacity(topk) : 0;
    const int n_wg = 128;
    // the exact tail's work buffer lives with the handle: its tickets are zeroed where it is allocated, not per pass
    Dev &exact_work = sv->exact_work;
    if (!exact_work.p) {
        if (!exact_work.alloc((size_t)pk_exact_work_bytes(n_wg, n_items))) return fail(ctx, PK_E_LAUNCH, "out of device memory (exact rows)");
        CK(pk_exact_work_init(st, exact_work.p, n_wg, n_items));
    }
    if (KC == 0) {
        // beyond the fused sweep (topk > 52 or rank > 256): every user through the exact fp64 row kernel
        DMat E(n_users, K);
        if (!E.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (E)");
        CK(spmm(ctx, Ts, V.p(), PK_VAL_F64, K, K, E.p(), K, all));
        hipLaunchKernelGGL(iota_i32_kernel, dim3((unsigned)((n_users + 255) / 256)), dim3(256), 0, st, n_users, lst.as<int32_t>(), cnt.as<int32_t>());
        CK(pk_score_exact_list_f64(st, n_wg, lst.as<int32_t>(), cnt.as<int32_t>(), n_items, K, V.p(), K, E.p(), K, seen_ptr, seen_idx, topk,
                                   out_i.as<int64_t>(), out_s.as<double>(), exact_work.p, nullptr));
        HIPCK(hipStreamSynchronize(st));
    } else {
        const bool approx = !out_scores && sv->have_v32;
        const int Kx = approx ? sv->Kx_full : K, ld32 = sv->ld32;
        DMat Ex(n_users, Kx);
        if (!Ex.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (E)");
        bool counters_zeroed = false;
        if (approx && sv->q20_img && topk <= 20) {      // (scoring.py: PACKED_MAX_TOPK — longer lists keep the fp32 image)
            // K4q: the packed image — E'[:, :K], the certified weight w in column K, zeros behind it
            Plan &P = Ts.plan;
            const size_t need = (size_t)P.n_slots * Kx * 8;
            if (need > P.partial.bytes && !P.partial.alloc(need)) return fail(ctx, PK_E_LAUNCH, "out of device memory (fold-in partials)");
            // ... and the two list counters of the pass (cnt2, below) zeroed by the fold-in's fix-up launch (scoring.py: fold_zeroes)
            CK(pk_fold_q20_zero(st, all.nt, P.task_row.as<int32_t>() + all.t0, P.task_begin.as<int64_t>() + all.t0,
                                P.task_end.as<int64_t>() + all.t0, P.task_slot.as<int32_t>() + all.t0, all.nl,
                                P.long_row.as<int32_t>() + all.l0, P.long_sb.as<int32_t>() + all.l0, P.long_se.as<int32_t>() + all.l0,
                                Ts.indices.as<int32_t>(), Ts.values.p, Ts.val_kind, sv->q20_img, sv->q20_tab.as<double>(), n_items, K, Kx,
                                Ex.p(), Kx, P.partial.as<double>(), cnt2.as<int32_t>(), 2));
            counters_zeroed = true;
        } else if (approx) CK(spmm(ctx, Ts, sv->V32.p, PK_VAL_F32, ld32, Kx, Ex.p(), Kx, all));
        else CK(spmm(ctx, Ts, V.p(), PK_VAL_F64, K, K, Ex.p(), Kx, all));
        const double *w = approx ? Ex.p() + K : nullptr;
        // the users' fragments and pruning bounds: built by the sweep's own waves from the rows of E when those are aligned
        // (scoring.py: SWEEP_FROM_ROWS — no packing launch, no packed copy), else by the packing kernel
        const bool from_rows = (Kx % 2 == 0) && (((uintptr_t)Ex.p()) % 16 == 0);
        Dev Ep, ub;
        if (!from_rows) {
            if (!Ep.alloc((size_t)pk_pack_elems(n_users, K) * 4) || !ub.alloc((size_t)n_users * 4))
                return fail(ctx, PK_E_LAUNCH, "out of device memory (E fragments)");
            CK(pk_pack_frag_bound_f32(st, n_users, K, Ex.p(), Kx, Ep.as<float>(), ub.as<float>(), w, approx ? Kx : 0, 1.2e-7));
        }
        if (filter_seen && !sv->have_tiles) {
            if (!sv->tiles.alloc(n1 * 8) || !sv->ntiles.alloc((size_t)n_users * 4)) return fail(ctx, PK_E_LAUNCH, "out of device memory (seen tiles)");
            CK(pk_seen_tiles_build(st, n_users, Ts.indptr.as<int64_t>(), Ts.indices.as<int32_t>(), 1, 0, sv->tiles.as<uint64_t>(), sv->ntiles.as<int32_t>()));
            sv->have_tiles = true;
            // dense masks for the head of the catalogue (ops.DeviceCSR.seen_dense: at most 256 tiles and 512 MB, not for
            // catalogues of more than 32 windows)
            const int64_t n_tiles_all = (n_items + 31) / 32, groups = (n_users + 31) / 32;
            int dt = (int)std::min<int64_t>(n_tiles_all, 256);
            while (dt > 32 && groups * dt * 128 > ((int64_t)512 << 20)) dt /= 2;
            if (n_tiles_all <= 32 * (int64_t)dt && sv->dense.alloc((size_t)pk_seen_dense_bytes(n_users, dt)) &&
                sv->skip.alloc((size_t)n_users * 4)) {
                CK(pk_seen_dense_build(st, n_users, Ts.indptr.as<int64_t>(), sv->tiles.as<uint64_t>(), sv->ntiles.as<int32_t>(), dt,
                                       sv->dense.as<uint32_t>(), sv->skip.as<int32_t>()));
                sv->dense_tiles = dt;
            }
        }
        const uint64_t *tiles = filter_seen ? sv->tiles.as<uint64_t>() : nullptr;
        const int32_t *ntiles = filter_seen ? sv->ntiles.as<int32_t>() : nullptr;
        int splits = ((n_users + 31) / 32) * 8 > 2048 ? 1 : pk_score_splits(n_users, KC);
        const int64_t n_pad = ((n_users + 31) / 32) * 32;
        // user sets that leave wave slots idle: head sweep + item splits seeded with its thresholds + merge (scoring.py)
        int32_t head_tiles = 0, splits2 = 0;
        CK(pk_score_two_phase_plan(n_users, n_items, KC, &head_tiles, &splits2));
        const int slots = head_tiles ? splits2 + 1 : splits;
        Dev state((size_t)pk_score_state_bytes(n_users, slots)), cs((size_t)slots * n_pad * KC * 4), ci((size_t)slots * n_pad * KC * 4);
        Dev ms(head_tiles ? (size_t)n_pad * KC * 4 : 0), mi(head_tiles ? (size_t)n_pad * KC * 4 : 0);
        if (!state.p || !cs.p || !ci.p || (head_tiles && (!ms.p || !mi.p))) return fail(ctx, PK_E_LAUNCH, "out of device memory (candidates)");
        const uint32_t *dense_p = (filter_seen && sv->dense_tiles) ? sv->dense.as<uint32_t>() : nullptr;
        const int32_t *skip_p = (filter_seen && sv->dense_tiles) ? sv->skip.as<int32_t>() : nullptr;
        // the users' side of the sweep entries: the rows of E with their error weights, or the packed fragments with their bounds
        const double *rows_p = from_rows ? Ex.p() : nullptr, *rows_w = from_rows ? w : nullptr;
        const int64_t rows_wld = (from_rows && approx) ? Kx : 0;
        if (head_tiles) {
            CK(pk_score_two_phase_f32(st, n_users, n_items, K, sv->Vp.as<float>(), Ep.as<float>(), ub.as<float>(), rows_p, Kx, rows_w,
                                      rows_wld, 1.2e-7, nullptr, seen_ptr, tiles, ntiles, KC, head_tiles, splits2, cs.as<float>(),
                                      ci.as<int32_t>(), ms.as<float>(), mi.as<int32_t>(), state.p, 0, sv->tile_bound.as<float>(),
                                      dense_p, skip_p, filter_seen ? sv->dense_tiles : 0));
            std::swap(cs, ms);      // the merged list is what the re-scoring takes: one list per user
            std::swap(ci, mi);
            splits = 1;
        } else {
            CK(pk_score_candidates_f32(st, n_users, n_items, K, sv->Vp.as<float>(), Ep.as<float>(), ub.as<float>(), rows_p, Kx, rows_w,
                                       rows_wld, 1.2e-7, nullptr, seen_ptr, tiles, ntiles, KC, splits, cs.as<float>(),
                                       ci.as<int32_t>(), state.p, 0, sv->tile_bound.as<float>(), dense_p, skip_p,
                                       filter_seen ? sv->dense_tiles : 0, nullptr));
        }
        // the lists of users to re-do are appended by the re-scoring kernel itself (scoring.py: fused lists): cnt2[0] counts
        // the re-fold list (lst), cnt2[1] the final list for the exact-row kernel (lst2)
        if (!counters_zeroed) CK(pk_zero_i32(st, cnt2.as<int32_t>(), 2));
        int32_t *c_refold = cnt2.as<int32_t>(), *c_final = cnt2.as<int32_t>() + 1;
        // (no out_perm: the lists are in serving order already; no user_norm: this pass runs without the settle tier)
        CK(pk_rescore_f64(st, n_users, nullptr, nullptr, n_users, n_items, K, V.p(), K, approx ? sv->V32.as<float>() : nullptr, approx ? ld32 : 0,
                          Ex.p(), Kx, w, approx ? Kx : 0, 0, seen_ptr, KC, splits, cs.as<float>(), ci.as<int32_t>(), topk, vmax,
                          out_i.as<int64_t>(), out_s.as<double>(), flags.as<int32_t>(),
                          approx ? lst.as<int32_t>() : lst2.as<int32_t>(), approx ? c_refold : c_final, 0,
                          approx ? sv->vnorm.as<float>() : nullptr, nullptr, nullptr));
        if (approx) {
            // the exact re-fold of the listed users on the product's own row tasks (scoring.py: ops.spmm_rows_list)
            // (even ranks; odd ones keep the one-workgroup-per-row kernel)
            if ((K & 1) == 0 && K >= 2) {
                Plan &P = Ts.plan;
                const size_t need = (size_t)P.n_slots * K * 8;
                if (need > P.partial.bytes && !P.partial.alloc(need)) return fail(ctx, PK_E_LAUNCH, "out of device memory (re-fold partials)");
                CK(pk_spmm_csr_rows_list_f64(st, n_users, lst.as<int32_t>(), c_refold, 0, P.row_first_task.as<int64_t>(), P.task_row.as<int32_t>(),
                                             P.task_begin.as<int64_t>(), P.task_end.as<int64_t>(), P.task_slot.as<int32_t>(), all.nl,
                                             P.long_row.as<int32_t>() + all.l0, P.long_sb.as<int32_t>() + all.l0, P.long_se.as<int32_t>() + all.l0,
                                             Ts.indices.as<int32_t>(), Ts.values.p, Ts.val_kind, V.p(), K, K, Ex.p(), Kx, P.partial.as<double>(),
                                             n_items, flags.as<int32_t>(), 7));
            } else
            CK(pk_fold_rows_f64(st, n_users, lst.as<int32_t>(), c_refold, 0, Ts.indptr.as<int64_t>(), Ts.indices.as<int32_t>(), Ts.values.p,
                                Ts.val_kind, V.p(), K, K, Ex.p(), Kx));
            CK(pk_rescore_f64(st, n_users, lst.as<int32_t>(), c_refold, n_users, n_items, K, V.p(), K, nullptr, 0, Ex.p(), Kx, w, Kx,
                              1, seen_ptr, KC, splits, cs.as<float>(), ci.as<int32_t>(), topk, vmax, out_i.as<int64_t>(), out_s.as<double>(),
                              flags.as<int32_t>(), lst2.as<int32_t>(), c_final, 0, nullptr, nullptr, nullptr));
        }
        CK(pk_score_exact_list_f64(st, n_wg, lst2.as<int32_t>(), c_final, n_items, K, V.p(), K, Ex.p(), Kx, seen_ptr, seen_idx, topk,
                                   out_i.as<int64_t>(), out_s.as<double>(), exact_work.p, nullptr));
        HIPCK(hipStreamSynchronize(st));   // every temporary above is still alive here
    }
    // serving order -> the caller's item ids on the device, then one transfer into the caller's array
    Dev ext((size_t)n_users * topk * 8);
    if (!ext.p) return fail(ctx, PK_E_LAUNCH, "out of device memory (outputs)");
    CK(pk_map_ids_i64(st, n_users * (int64_t)topk, out_i.as<int64_t>(), sv->inv64.as<int64_t>(), n_items, ext.as<int64_t>()));
    CK(S.to_host(ext.p, out_idx, (size_t)n_users * topk * 8));
    if (out_scores) CK(S.to_host(out_s.p, out_scores, (size_t)n_users * topk * 8));
    return PK_OK;
}

}  // namespace

extern "C" int pk_serving_create(pk_ctx *ctx, int64_t n_items, int32_t K, const double *V_host, pk_mat *T, pk_serving **out) {
    if (!ctx || !T || !out) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    (void)hipSetDevice(ctx->device);
    *out = nullptr;
    if (n_items != T->A.n_cols) return fail(ctx, PK_E_INVALID, "pk_score_topk: test matrix and item factors disagree on the number of items");
    if (K < 1 || K > 8192 || !V_host) return fail(ctx, PK_E_INVALID, "pk_score_topk: bad arguments");
    std::unique_ptr<pk_serving> sv(new pk_serving());
    const int rc = serving_build(ctx, sv.get(), n_items, K, V_host, T);
    if (rc != PK_OK) return rc;
    *out = sv.release();
    return PK_OK;
}

extern "C" int pk_serving_score(pk_ctx *ctx, pk_serving *sv, int32_t topk, int32_t filter_seen, int64_t *out_idx, double *out_scores) {
    if (!ctx || !sv) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    (void)hipSetDevice(ctx->device);
    return serving_score(ctx, sv, topk, filter_seen, out_idx, out_scores);
}

extern "C" void pk_serving_free(pk_ctx *ctx, pk_serving *sv) {
    if (!sv) return;
    if (ctx) {
        std::lock_guard<std::mutex> lock(ctx->mu);
        PoolScope pool_scope(ctx);
        (void)hipStreamSynchronize(ctx->stream);
        delete sv;
    } else {
        delete sv;
    }
}

extern "C" int pk_score_topk(pk_ctx *ctx, int64_t n_items, int32_t K, const double *V_host, pk_mat *T, int32_t topk,
                             int32_t filter_seen, int64_t *out_idx, double *out_scores) {
    if (!ctx || !T) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    (void)hipSetDevice(ctx->device);
    if (n_items != T->A.n_cols) return fail(ctx, PK_E_INVALID, "pk_score_topk: test matrix and item factors disagree on the number of items");
    if (K < 1 || K > 8192 || !V_host || !out_idx || topk < 1) return fail(ctx, PK_E_INVALID, "pk_score_topk: bad arguments");
    if (topk > n_items) return fail(ctx, PK_E_INVALID, "kth(=%lld) out of bounds (%lld)", (long long)(n_items - topk), (long long)n_items);
    pk_serving sv;
    int rc = serving_build(ctx, &sv, n_items, K, V_host, T);
    if (rc == PK_OK) rc = serving_score(ctx, &sv, topk, filter_seen, out_idx, out_scores);
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// ------------------------------------------------------------------------------------------------------------
// pk_hooi: polara_amd/tucker.py::hooi restated (CoffeeModel.build -> lib/tensor.py:37-96)
// ------------------------------------------------------------------------------------------------------------
namespace {

struct ModePlan {     // nnz ordered by one mode + the wave-task plan of pk_ttm_f64
    Csr rows;         // only indptr + plan are used (n_rows = size of the output mode)
    Dev idx_u, idx_v, vals;
    bool ones = true;
};

int make_mode_plan(pk_ctx *ctx, int64_t nnz, const int64_t *idx, const double *vals, const int64_t shape[3], int mode0, int mode_u,
                   int mode_v, ModePlan &mp) {
    const int64_t n0 = shape[mode0];
    std::vector<int64_t> indptr((size_t)n0 + 1, 0);
    for (int64_t p = 0; p < nnz; ++p) indptr[(size_t)idx[3 * p + mode0] + 1] += 1;
    for (int64_t r = 0; r < n0; ++r) indptr[(size_t)r + 1] += indptr[(size_t)r];
    std::vector<int64_t> cursor(indptr.begin(), indptr.end() - 1);
    std::vector<int32_t> iu((size_t)std::max<int64_t>(nnz, 1)), iv((size_t)std::max<int64_t>(nnz, 1));
    std::vector<double> vv;
    mp.ones = true;
    if (vals) for (int64_t p = 0; p < nnz; ++p) if (vals[p] != 1.0) { mp.ones = false; break; }
    if (!mp.ones) vv.resize((size_t)nnz);
    for (int64_t p = 0; p < nnz; ++p) {          // stable counting sort by the output mode (nnz order kept inside a row)
        const int64_t d = cursor[(size_t)idx[3 * p + mode0]]++;
        iu[(size_t)d] = (int32_t)idx[3 * p + mode_u];
        iv[(size_t)d] = (int32_t)idx[3 * p + mode_v];
        if (!mp.ones) vv[(size_t)d] = vals[p];
    }
    Csr &R = mp.rows;
    R.n_rows = n0; R.n_cols = 1; R.nnz = nnz;
    const size_t n1 = (size_t)std::max<int64_t>(nnz, 1);
    if (!R.indptr.alloc(((size_t)n0 + 1) * 8) || !mp.idx_u.alloc(n1 * 4) || !mp.idx_v.alloc(n1 * 4) || (!mp.ones && !mp.vals.alloc(n1 * 8)))
        return fail(ctx, PK_E_LAUNCH, "out of device memory (tensor plan)");
    hipStream_t st = ctx->stream;
    HIPCK(hipMemcpyAsync(R.indptr.p, indptr.data(), ((size_t)n0 + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz) {
        HIPCK(hipMemcpyAsync(mp.idx_u.p, iu.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(mp.idx_v.p, iv.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        if (!mp.ones) HIPCK(hipMemcpyAsync(mp.vals.p, vv.data(), (size_t)nnz * 8, hipMemcpyHostToDevice, st));
    }
    HIPCK(hipStreamSynchronize(st));
    return build_plan(ctx, R, 256);
}

// res[n0 x (ra * rb)] = sum over the nnz of row i0 of val * u[i_u, :] (x) v[i_v, :]
int ttm(pk_ctx *ctx, ModePlan &mp, const DMat &u, const DMat &v, DMat &res) {
    Plan &P = mp.rows.plan;
    const int ra = u.l, rb = v.l;
    res = DMat(mp.rows.n_rows, ra * rb);
    if (!res.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (ttm)");
    const size_t need = (size_t)P.n_slots * ra * rb * 8;
    if (need > P.partial.bytes && !P.partial.alloc(need)) return fail(ctx, PK_E_LAUNCH, "out of device memory (ttm partials)");
    CK(pk_ttm_f64(ctx->stream, P.n_tasks, P.task_row.as<int32_t>(), P.task_begin.as<int64_t>(), P.task_end.as<int64_t>(),
                  P.task_slot.as<int32_t>(), P.n_long, P.long_row.as<int32_t>(), P.long_sb.as<int32_t>(), P.long_se.as<int32_t>(),
                  mp.idx_u.as<int32_t>(), mp.idx_v.as<int32_t>(), mp.ones ? nullptr : mp.vals.as<double>(), u.p(), u.l, ra, v.p(), v.l, rb,
                  res.p(), res.l, P.partial.as<double>()));
    return PK_OK;
}

// top-r left singular vectors / values of dense M (tucker.left_svd, single process): U [n x r], s (host), Vt [r x m] if asked
// eigh of the Gram matrix G started from the previous HOOI iteration's eigenvectors Q of the same mode (tucker._eigh_warm):
// G' = Q^T G Q is nearly diagonal, the Jacobi sweeps on it stop after 3-4 instead of ~10, and Q C' are G's eigenvectors
int eigh_warm(Solver &S, const DMat &G, DMat *Q, std::vector<double> &lam, DMat &C, Dev &lam_dev) {
    pk_ctx *ctx = S.ctx;
    if (!Q || !Q->ok() || Q->n != G.n || Q->l != G.l || Q->n < 1) {
        CK(S.eigh(G, lam, C, lam_dev));
    } else {
        DMat GQ, G1, G1t, Gs, C1;
        CK(S.tsmm(G, *Q, GQ));
        CK(S.gram(*Q, GQ, G1));
        G1t = DMat(G1.n, G1.l);
        if (!G1t.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (eigh_warm)");
        hipLaunchKernelGGL(transpose_small_kernel, dim3((unsigned)((G1.l * G1.l + 255) / 256)), dim3(256), 0, S.st, G1.l, G1.p(), G1t.p());
        CK(S.axpbypcz(0.5, G1, 0.5, &G1t, 0.0, nullptr, Gs));
        CK(S.eigh(Gs, lam, C1, lam_dev));
        CK(S.tsmm(*Q, C1, C));
    }
    if (Q) CK(S.col_slice(C, 0, C.l, *Q));
    return PK_OK;
}

// the r leading eigenpairs of the Gram matrix G: lam (host, >= r values), W [n x r] (columns).  pk_eigh_top_f64 where it
// applies and passes its own check (tucker._eigh_lead), else the warm-started Jacobi route above
int eigh_lead(Solver &S, const DMat &G, int r, DMat *warm, std::vector<double> &lam, DMat &W) {
    pk_ctx *ctx = S.ctx;
    const int n = G.l;
    if (pk_eigh_top_supported(n, r) && 2 * r <= n) {
        DMat R(r, n);
        Dev lam_dev, info, work;
        if (!R.ok() || !lam_dev.alloc((size_t)r * 8) || !info.alloc(8) || !work.alloc((size_t)pk_eigh_top_work_bytes(n)))
            return fail(ctx, PK_E_LAUNCH, "out of device memory (eigh_lead)");
        CK(pk_eigh_top_f64(S.st, n, G.p(), n, r, R.p(), n, lam_dev.as<double>(), work.p, info.as<int32_t>()));
        int32_t verdict = 0;
        CK(S.to_host(info.p, &verdict, sizeof(verdict)));
        if (verdict == 1) {
            W = DMat(n, r);
            if (!W.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (eigh_lead)");
            hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)(((size_t)r * n + 255) / 256)), dim3(256), 0, S.st, (int64_t)r, n, R.p(), W.p());
            lam.resize((size_t)r);
            return S.to_host(lam_dev.p, lam.data(), (size_t)r * 8);
        }
    }
    DMat C;
    Dev lam_dev;
    CK(eigh_warm(S, G, warm, lam, C, lam_dev));
    return S.col_slice(C, 0, r, W);
}

int left_svd(Solver &S, const DMat &M, int r, DMat &U, std::vector<double> &s, DMat *Vt, DMat *warm = nullptr) {
    pk_ctx *ctx = S.ctx;
    const int64_t n = M.n;
    const int m = M.l;
    if (r > std::min<int64_t>(n, m)) return fail(ctx, PK_E_INVALID, "rank %d exceeds min(shape)=%lld", r, (long long)std::min<int64_t>(n, m));
    std::vector<double> lam;
    Dev lam_dev;
    s.assign((size_t)r, 0.0);
    if (n >= m) {
        DMat G, W, Ur, Gu;
        CK(S.gram(M, M, G));
        CK(eigh_lead(S, G, r, warm, lam, W));
        std::vector<double> inv((size_t)r);
        for (int i = 0; i < r; ++i) { s[(size_t)i] = std::sqrt(std::max(lam[(size_t)i], 0.0)); inv[(size_t)i] = s[(size_t)i] > 0 ? 1.0 / s[(size_t)i] : 0.0; }
        CK(S.tsmm(M, W, Ur));
        CK(S.scale_cols_host(Ur, inv));
        // one Newton-Schulz step: U <- U (1.5 I - 0.5 U^T U)
        CK(S.gram(Ur, Ur, Gu));
        std::vector<double> g((size_t)r * r);
        CK(S.to_host(Gu.p(), g.data(), g.size() * 8));
        for (int i = 0; i < r; ++i) for (int j = 0; j < r; ++j) g[(size_t)i * r + j] = (i == j ? 1.5 : 0.0) - 0.5 * g[(size_t)i * r + j];
        DMat Cn(r, r);
        CK(S.upload(g.data(), Cn.p(), g.size() * 8));
        CK(S.tsmm(Ur, Cn, U));
        if (Vt) {
            *Vt = DMat(r, m);
            hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)(((size_t)m * r + 255) / 256)), dim3(256), 0, S.st, (int64_t)m, r, W.p(), Vt->p());
        }
    } else {
        DMat Mt(m, (int)n), G, C;
        hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)(((size_t)n * m + 255) / 256)), dim3(256), 0, S.st, n, m, M.p(), Mt.p());
        CK(S.gram(Mt, Mt, G));
        CK(eigh_warm(S, G, warm, lam, C, lam_dev));
        CK(S.col_slice(C, 0, r, U));
        for (int i = 0; i < r; ++i) s[(size_t)i] = std::sqrt(std::max(lam[(size_t)i], 0.0));
        if (Vt) {
            *Vt = DMat(r, m);
            CK(pk_dgemm_small_f64(S.st, 1, 0, r, m, (int)n, U.p(), U.l, M.p(), M.l, Vt->p(), m));    // U^T M = diag(s) V^T
            std::vector<double> h((size_t)r * m);
            CK(S.to_host(Vt->p(), h.data(), h.size() * 8));
            for (int i = 0; i < r; ++i) { const double inv = s[(size_t)i] > 0 ? 1.0 / s[(size_t)i] : 0.0; for (int j = 0; j < m; ++j) h[(size_t)i * m + j] *= inv; }
            CK(S.upload(h.data(), Vt->p(), h.size() * 8));
        }
    }
    return PK_OK;
}

}  // namespace

extern "C" int pk_hooi(pk_ctx *ctx, int64_t nnz, const int64_t *idx_host, const double *vals_host, const int64_t *shape,
                       const int32_t *mlrank, int32_t num_iters, double growth_tol, const double *u1_start, const double *u2_start,
                       uint64_t seed, double *u0_out, double *u1_out, double *u2_out, double *core_out, double *trace_out,
                       int32_t *iters_out) {
    if (!ctx) return PK_E_INVALID;
    std::lock_guard<std::mutex> lock(ctx->mu);
    PoolScope pool_scope(ctx);
    (void)hipSetDevice(ctx->device);
    if (nnz < 1 || !idx_host || !shape || !mlrank || !u0_out || !u1_out || !u2_out || !core_out)
        return fail(ctx, PK_E_INVALID, "pk_hooi: bad arguments");
    const int64_t n0 = shape[0], n1 = shape[1], n2 = shape[2];
    const int r0 = mlrank[0], r1 = mlrank[1], r2 = mlrank[2];
    if (n0 < 1 || n1 < 1 || n2 < 1 || r0 < 1 || r1 < 1 || r2 < 1 || r0 > n0 || r1 > n1 || r2 > n2)
        return fail(ctx, PK_E_INVALID, "pk_hooi: ranks must satisfy 1 <= r_k <= n_k");
    if ((int64_t)r2 * r1 > 1024 || (int64_t)r2 * r0 > 1024 || (int64_t)r1 * r0 > 1024)
        return fail(ctx, PK_E_UNSUPPORTED, "pk_hooi: a product of two ranks beyond 1024 (pk_ttm_f64 / the dense kernels)");
    for (int64_t p = 0; p < nnz; ++p)
        for (int k = 0; k < 3; ++k)
            if (idx_host[3 * p + k] < 0 || idx_host[3 * p + k] >= shape[k]) return fail(ctx, PK_E_INVALID, "pk_hooi: index out of bounds");
    if (num_iters <= 0) num_iters = 25;
    Solver S{ctx, ctx->stream, Dev()};
    // The three mode products of lib/tensor.py:70,74,78 in FACTORED form (polara_amd/tucker.py::factored_products): the
    // tensor as two CSR unfoldings, M0 [(n0 L) x n1] with row i0 L + l and M1 [(n1 L) x n0] with row i1 L + l (L = n2, the
    // feedback mode); SpMM gathers W0 = M0 u1, W1 = M1 u0, then dense contractions on the fp64 matrix cores (tsmm against
    // kron(u2, I), one gram for the feedback mode).  Context option "hooi_ttm" = 1 keeps the per-entry kernel (pk_ttm_f64, dttm_seq restated).
    const bool factored = ctx->opt.hooi_ttm == 0;
    const int64_t L = n2;
    ModePlan mp0, mp1, mp2;
    std::unique_ptr<pk_mat> M0, M1;
    if (factored) {
        std::vector<int64_t> rr((size_t)nnz), cc((size_t)nnz);
        std::vector<double> ones;
        const double *vals = vals_host;
        if (!vals) { ones.assign((size_t)nnz, 1.0); vals = ones.data(); }
        pk_mat *tmp = nullptr;
        for (int64_t p = 0; p < nnz; ++p) { rr[(size_t)p] = idx_host[3 * p] * L + idx_host[3 * p + 2]; cc[(size_t)p] = idx_host[3 * p + 1]; }
        CK(mat_from_coo_impl(ctx, n0 * L, n1, nnz, rr.data(), cc.data(), 1, vals, PK_VAL_F64, &tmp));
        M0.reset(tmp);
        for (int64_t p = 0; p < nnz; ++p) { rr[(size_t)p] = idx_host[3 * p + 1] * L + idx_host[3 * p + 2]; cc[(size_t)p] = idx_host[3 * p]; }
        CK(mat_from_coo_impl(ctx, n1 * L, n0, nnz, rr.data(), cc.data(), 1, vals, PK_VAL_F64, &tmp));
        M1.reset(tmp);
    } else {
        // (output mode ; first matrix mode ; second matrix mode) as in lib/tensor.py:70,74,78
        CK(make_mode_plan(ctx, nnz, idx_host, vals_host, shape, 0, 2, 1, mp0));
        CK(make_mode_plan(ctx, nnz, idx_host, vals_host, shape, 1, 2, 0, mp1));
        CK(make_mode_plan(ctx, nnz, idx_host, vals_host, shape, 2, 1, 0, mp2));
    }
    // kron(u2, I_r) [L r x r2 r] on the device (u2 is L x r2: a few dozen numbers through the host)
    auto kron_u2 = [&](const DMat &u2m, int r, DMat &K) -> int {
        std::vector<double> h((size_t)L * r2), k((size_t)L * r * r2 * r, 0.0);
        CK(S.to_host(u2m.p(), h.data(), h.size() * 8));
        for (int64_t l = 0; l < L; ++l)
            for (int j = 0; j < r2; ++j)
                for (int c = 0; c < r; ++c) k[((size_t)l * r + c) * ((size_t)r2 * r) + (size_t)j * r + c] = h[(size_t)l * r2 + j];
        K = DMat(L * r, r2 * r);
        if (!K.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (kron)");
        return S.upload(k.data(), K.p(), k.size() * 8);
    };
    DMat W1;                    // [n1 x L r0]: the gathers of mode 1, reused by mode 2
    auto product = [&](int mode, const DMat &a0, const DMat &a1, const DMat &a2, DMat &res) -> int {
        if (!factored) return mode == 0 ? ttm(ctx, mp0, a2, a1, res) : mode == 1 ? ttm(ctx, mp1, a2, a0, res) : ttm(ctx, mp2, a1, a0, res);
        if (mode == 0) {
            DMat W0(n0 * L, r1), K;
            if (!W0.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (W0)");
            CK(spmm_full(ctx, M0->A, a1, W0));
            W0.n = n0; W0.l = (int)(L * r1);                      // the same memory read as [n0 x L r1]
            CK(kron_u2(a2, r1, K));
            return S.tsmm(W0, K, res);
        }
        if (mode == 1) {
            DMat K;
            W1 = DMat(n1 * L, r0);
            if (!W1.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (W1)");
            CK(spmm_full(ctx, M1->A, a0, W1));
            W1.n = n1; W1.l = (int)(L * r0);
            CK(kron_u2(a2, r0, K));
            return S.tsmm(W1, K, res);
        }
        // mode 2: res[l, j r0 + k] = (u1^T W1)[j, l r0 + k]
        DMat G;
        CK(S.gram(a1, W1, G));
        std::vector<double> g((size_t)r1 * L * r0), t((size_t)L * r1 * r0);
        CK(S.to_host(G.p(), g.data(), g.size() * 8));
        for (int j = 0; j < r1; ++j)
            for (int64_t l = 0; l < L; ++l)
                for (int k = 0; k < r0; ++k) t[((size_t)l * r1 + j) * r0 + k] = g[(size_t)j * (L * r0) + (size_t)l * r0 + k];
        res = DMat(L, r1 * r0);
        if (!res.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (mode-2 product)");
        return S.upload(t.data(), res.p(), t.size() * 8);
    };
    DMat warm0, warm1, warm2;   // the previous iteration's eigenvectors per mode (eigh_warm)
    DMat u0, u1(n1, r1), u2(n2, r2);
    if (!u1.ok() || !u2.ok()) return fail(ctx, PK_E_LAUNCH, "out of device memory (factors)");
    if (u1_start && u2_start) {       // the caller's start (the reference draws it from NumPy's RandomState + LAPACK QR, tensor.py:57-63)
        CK(S.upload(u1_start, u1.p(), (size_t)n1 * r1 * 8));
        CK(S.upload(u2_start, u2.p(), (size_t)n2 * r2 * 8));
    } else {
        DMat a, b;
        CK(S.randn(n1, r1, seed, a));
        CK(S.randn(n2, r2, seed + 1, b));
        CK(S.orthonormalize(a, nullptr, seed + 2, u1));
        CK(S.orthonormalize(b, nullptr, seed + 3, u2));
    }
    double g_old = 0.0;
    std::vector<double> ss, s_tmp;
    DMat vv;
    int it = 0;
    for (; it < num_iters; ++it) {
        DMat T0, T1, T2, n0f, n1f, n2f;
        CK(product(0, u0, u1, u2, T0));
        CK(left_svd(S, T0, r0, n0f, s_tmp, nullptr, &warm0));
        u0 = std::move(n0f);
        CK(product(1, u0, u1, u2, T1));
        CK(left_svd(S, T1, r1, n1f, s_tmp, nullptr, &warm1));
        u1 = std::move(n1f);
        CK(product(2, u0, u1, u2, T2));
        CK(left_svd(S, T2, r2, n2f, ss, &vv, &warm2));
        u2 = std::move(n2f);
        double g_new = 0.0;
        for (double v : ss) g_new += v * v;
        g_new = std::sqrt(g_new);
        const double growth = (g_new - g_old) / g_new;
        g_old = g_new;
        if (trace_out) trace_out[it] = g_new;
        if (growth < growth_tol) { ++it; break; }
    }
    if (iters_out) *iters_out = it;
    CK(S.to_host(u0.p(), u0_out, (size_t)n0 * r0 * 8));
    CK(S.to_host(u1.p(), u1_out, (size_t)n1 * r1 * 8));
    CK(S.to_host(u2.p(), u2_out, (size_t)n2 * r2 * 8));
    // core[a, b, c] = ss[c] * vv[c, b * r0 + a]   ((ss * vv).reshape(r2, r1, r0).transpose(2, 1, 0), tensor.py:91-93)
    std::vector<double> vh((size_t)r2 * r1 * r0);
    CK(S.to_host(vv.p(), vh.data(), vh.size() * 8));
    for (int a = 0; a < r0; ++a)
        for (int b = 0; b < r1; ++b)
            for (int c = 0; c < r2; ++c) core_out[((size_t)a * r1 + b) * r2 + c] = ss[(size_t)c] * vh[(size_t)c * r1 * r0 + (size_t)b * r0 + a];
    return PK_OK;
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp): the runtime loads a code object at the first
// launch of one of its kernels — or when a kernel's attributes are asked for, which costs no launch
hipError_t pk_tu_load_driver() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&transpose_small_kernel));
}
