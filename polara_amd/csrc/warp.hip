// LightFM's WARP model (Kula 2015; Weston et al. 2011) on the conflict-free blocked schedule of BPR (polara_amd/warp.py): rank k
// plus a bias, per-parameter adagrad, item representations q_i = a_i E_id[i] + S_i with S = F_lab E_lab the image of the label
// embeddings.  A sample touches one user row and the identity rows of the positive and of the violating candidate; candidates
// are drawn inside the positive's own item part, so the blocks of a stratum share no row they write and one launch sweeps them
// side by side, each block sequentially by one lane group.  The label embeddings are shared between blocks: they are read-only
// during a stratum (S is formed by a launch before it), every block adds the label gradients of its own items into its own rows
// of G, and a launch after the stratum sums G over every label's items in ascending item order and takes one adagrad step per
// label.  No atomics, no flags, no grid barrier: stream order is the only synchronisation.  The arithmetic of a sample, the draw
// stream and the loss table are spelled out in polara_hip.h.  gfx950 only (wave = 64).
#include "pk_common.h"

// every product and sum below is rounded on its own, as NumPy rounds them (the library is built with contraction on)
#pragma clang fp contract(off)

#include "blocked_sweep.h"            // after the pragma: the shared helpers are compiled without contraction too

#define WARP_MAX_RANK 63            // k + 1 columns (the bias) in one wave
#define WARP_THREADS 64             // one wave per workgroup, as PMF_THREADS: a block's sweep is a chain of dependent loads
#define WARP_BATCH 4                // candidate rows whose loads are issued together (KPMF_BATCH)

// ---- the candidates of an epoch -----------------------------------------------------------------------------------------------
// one thread per (position, draw): a candidate that lies in the user's row is stored as -1
__global__ __launch_bounds__(256) void warp_draw_kernel(int64_t total, int D, const int32_t *__restrict__ users,
                                                        const int32_t *__restrict__ items, const int64_t *__restrict__ perm,
                                                        const int32_t *__restrict__ item_order, const int32_t *__restrict__ item_part,
                                                        const int64_t *__restrict__ item_ptr, const int64_t *__restrict__ indptr,
                                                        const int32_t *__restrict__ indices, uint64_t key, int32_t *__restrict__ cand) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= total) return;
    const int64_t p = x / D;
    const int t = (int)(x - p * D);
    const int32_t u = users[p], c = item_part[items[p]];
    const int64_t lo_c = item_ptr[c];
    const uint64_t n_c = (uint64_t)(item_ptr[c + 1] - lo_c);
    const int64_t r1 = indptr[u + 1];
    const int32_t j = pair_draw_in_part(item_order, lo_c, n_c, pk_mix64(key + 64ull * (uint64_t)perm[p] + (uint64_t)t) >> 32);
    cand[x] = pair_row_holds(indices, indptr[u], r1, j) ? -1 : j;
}

extern "C" int pk_warp_draw_candidates(void *stream, int64_t nnz, int64_t n_users, int64_t n_items, int32_t blocks, int32_t max_sampled,
                                       const int32_t *users_dev, const int32_t *items_dev, const int64_t *perm_dev,
                                       const int32_t *item_order_dev, const int32_t *item_part_dev, const int64_t *item_ptr_dev,
                                       const int64_t *indptr_dev, const int32_t *indices_dev, uint32_t seed, uint32_t epoch,
                                       int32_t *cand_dev) {
    const int rc = pair_draw_check("pk_warp_draw_candidates", nnz, n_users, n_items, blocks, max_sampled, PK_WARP_MAX_SAMPLED,
                                   item_order_dev && item_part_dev && item_ptr_dev && indptr_dev,
                                   nnz == 0 || (users_dev && items_dev && perm_dev && indices_dev && cand_dev));
    if (rc != PK_OK) return rc;
    if (nnz == 0) return PK_OK;
    const int64_t total = nnz * max_sampled;
    hipLaunchKernelGGL(warp_draw_kernel, dim3((unsigned)pk_ceil_div(total, 256)), dim3(256), 0, pk_stream(stream), total, (int)max_sampled,
                       users_dev, items_dev, perm_dev, item_order_dev, item_part_dev, item_ptr_dev, indptr_dev, indices_dev,
                       pair_stream_key(seed, epoch), cand_dev);
    PK_CHECK_LAUNCH("warp_draw_kernel");
    return PK_OK;
}

// ---- the label embeddings -------------------------------------------------------------------------------------------------------
// the item features F_lab = diag(a) one_hot as CSR (rows: items) and CSC (columns: labels, items ascending), and what they act on
struct WarpFeatures {
    int64_t n_items, n_labels;
    const double *a;                    // [n_items]: the weight of an item's identity column and of each of its labels
    const int64_t *row_ptr, *col_ptr;
    const int32_t *row_idx, *col_idx;
    const double *row_val, *col_val;
    double *L, *AL;                     // E_lab and its adagrad state [n_labels x cols]
    int64_t ldl, ldal;
    double *S, *G;                      // the image F_lab E_lab and the items' label gradients [n_items x cols]
    int64_t lds, ldg;
};

// S[i] = (+0.0 + v1 * L[l1]) + v2 * L[l2] + ... over row i of F_lab in storage order, one thread per (item, column); with
// `zero_g` the thread clears its cell of G as well (what the stratum before left there has been consumed by its label step)
__global__ __launch_bounds__(256) void warp_image_kernel(WarpFeatures f, int cols, bool zero_g) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= f.n_items * cols) return;
    const int64_t i = x / cols;
    const int c = (int)(x - i * cols);
    double acc = 0.0;
    for (int64_t e = f.row_ptr[i]; e < f.row_ptr[i + 1]; ++e) acc = acc + f.row_val[e] * f.L[(int64_t)f.row_idx[e] * f.ldl + c];
    f.S[i * f.lds + c] = acc;
    if (zero_g) f.G[i * f.ldg + c] = 0.0;
}

// g_l = (+0.0 + v1 * G[i1]) + v2 * G[i2] + ... over column l of F_lab (items ascending), then the adagrad step on E_lab[l]: one
// thread per (label, column).  G is only read here: items carry several labels, so it is cleared by the launches around this one.
__global__ __launch_bounds__(256) void warp_label_step_kernel(WarpFeatures f, int cols, double lr) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= f.n_labels * cols) return;
    const int64_t l = x / cols;
    const int c = (int)(x - l * cols);
    double g = 0.0;
    for (int64_t e = f.col_ptr[l]; e < f.col_ptr[l + 1]; ++e) g = g + f.col_val[e] * f.G[(int64_t)f.col_idx[e] * f.ldg + c];
    const double A = f.AL[l * f.ldal + c];
    const double step = lr / sqrt(A);
    f.L[l * f.ldl + c] = f.L[l * f.ldl + c] - step * g;
    f.AL[l * f.ldal + c] = A + g * g;
}

__global__ __launch_bounds__(256) void warp_zero_kernel(int64_t n, int cols, double *__restrict__ G, int64_t ldg) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n * cols) return;
    const int64_t i = x / cols;
    G[i * ldg + (x - i * cols)] = 0.0;
}

static unsigned warp_cells_grid(int64_t rows, int cols) { return (unsigned)pk_ceil_div(rows * cols > 0 ? rows * cols : 1, 256); }

static int warp_launch_image(hipStream_t st, const WarpFeatures &f, int cols, bool zero_g) {
    hipLaunchKernelGGL(warp_image_kernel, dim3(warp_cells_grid(f.n_items, cols)), dim3(256), 0, st, f, cols, zero_g);
    PK_CHECK_LAUNCH("warp_image_kernel");
    return PK_OK;
}

static int warp_launch_label_step(hipStream_t st, const WarpFeatures &f, int cols, double lr) {
    if (f.n_labels == 0) return PK_OK;
    hipLaunchKernelGGL(warp_label_step_kernel, dim3(warp_cells_grid(f.n_labels, cols)), dim3(256), 0, st, f, cols, lr);
    PK_CHECK_LAUNCH("warp_label_step_kernel");
    return PK_OK;
}

static int warp_launch_zero(hipStream_t st, const WarpFeatures &f, int cols) {
    hipLaunchKernelGGL(warp_zero_kernel, dim3(warp_cells_grid(f.n_items, cols)), dim3(256), 0, st, f.n_items, cols, f.G, f.ldg);
    PK_CHECK_LAUNCH("warp_zero_kernel");
    return PK_OK;
}

extern "C" int pk_warp_label_image_f64(void *stream, int32_t rank, int64_t n_items, int64_t n_labels, const int64_t *row_ptr_dev,
                                       const int32_t *row_idx_dev, const double *row_val_dev, const double *L_dev, int64_t ldl,
                                       double *S_dev, int64_t lds) {
    PK_REQUIRE(rank >= 1 && rank <= WARP_MAX_RANK, "pk_warp_label_image_f64: rank %d outside 1..%d", (int)rank, WARP_MAX_RANK);
    const int cols = rank + 1;
    PK_REQUIRE(n_items >= 1 && n_items < ((int64_t)1 << 31) && n_labels >= 0 && row_ptr_dev && S_dev && (n_labels == 0 || L_dev) &&
                   ldl >= cols && lds >= cols,
               "pk_warp_label_image_f64: bad arguments");
    WarpFeatures f = {};
    f.n_items = n_items, f.n_labels = n_labels;
    f.row_ptr = row_ptr_dev, f.row_idx = row_idx_dev, f.row_val = row_val_dev;
    f.L = const_cast<double *>(L_dev), f.ldl = ldl, f.S = S_dev, f.lds = lds;
    return warp_launch_image(pk_stream(stream), f, cols, false);
}

extern "C" int pk_warp_label_step_f64(void *stream, int32_t rank, int64_t n_items, int64_t n_labels, const int64_t *col_ptr_dev,
                                      const int32_t *col_idx_dev, const double *col_val_dev, double *G_dev, int64_t ldg, double *L_dev,
                                      int64_t ldl, double *AL_dev, int64_t ldal, double learning_rate) {
    PK_REQUIRE(rank >= 1 && rank <= WARP_MAX_RANK, "pk_warp_label_step_f64: rank %d outside 1..%d", (int)rank, WARP_MAX_RANK);
    const int cols = rank + 1;
    PK_REQUIRE(n_items >= 1 && n_items < ((int64_t)1 << 31) && n_labels >= 0 && n_labels < ((int64_t)1 << 31) && col_ptr_dev && G_dev &&
                   (n_labels == 0 || (L_dev && AL_dev && L_dev != AL_dev)) && ldg >= cols && ldl >= cols && ldal >= cols,
               "pk_warp_label_step_f64: bad arguments");
    WarpFeatures f = {};
    f.n_items = n_items, f.n_labels = n_labels;
    f.col_ptr = col_ptr_dev, f.col_idx = col_idx_dev, f.col_val = col_val_dev;
    f.L = L_dev, f.AL = AL_dev, f.ldl = ldl, f.ldal = ldal, f.G = G_dev, f.ldg = ldg;
    hipStream_t st = pk_stream(stream);
    const int rc = warp_launch_label_step(st, f, cols, learning_rate);
    return rc != PK_OK ? rc : warp_launch_zero(st, f, cols);
}

// ---- the sweep --------------------------------------------------------------------------------------------------------------
struct WarpArgs {
    int B, rank, D;
    const int64_t *block_ptr;
    const int32_t *users, *items, *cand;
    const double *table;                // [D]: the weight of a violator found at draw t
    double *P, *E, *AP, *AE;
    int64_t ldp, lde, ldap, ldae;
    double lr;
    const double *a, *S;                // FEAT only
    double *G;
    int64_t lds, ldg;
    int64_t *counts;                    // [3][B * B]: trained, quiet, draws of every block
};

// W lanes per block, 64 / W blocks per wave; lane c holds column c of the k + 1 (column k: the constant 1 of P, the bias of E).
// The loop over the samples runs to the longest block of the wave, the loop over a sample's candidates until no group of the
// wave is still looking, both with every lane active (the butterfly reads its neighbours); a group past the end of its block,
// or one that has found its violator, holds no candidate: it computes on zeros, loads nothing and stores nothing.  All lanes of
// a group see the same x_neg (group_sum), so a group's decisions are uniform.
// Sample t + 1's user row and positive row, with their adagrad state, are loaded while sample t is computed — unless one of
// them is a row sample t writes, whose new value is then forwarded in registers: the user row, and the positive row from the
// positive or from the violator of sample t.  Candidate rows are loaded when their sample is reached, WARP_BATCH at a time,
// behind the stores of the sample before.
template <int W, bool FEAT>
__global__ __launch_bounds__(WARP_THREADS) void warp_stratum_kernel(WarpArgs a, int stratum) {
    int c;
    const int64_t b = pk_sweep_lanes<W>(c);
    const bool qcol = c <= a.rank, pcol = c < a.rank;
    int64_t t0, len;
    const int64_t maxlen = pk_sweep_range<W>(a.B, a.block_ptr, stratum, b, t0, len);
    const int D = a.D;

    auto sample = [&](int64_t t, int &u, int &i) {
        u = i = -1;
        if (t < len) {
            u = a.users[t0 + t];
            i = a.items[t0 + t];
        }
    };
    auto row = [&](const double *X, int64_t ld, int r) { return (r >= 0 && qcol) ? X[(int64_t)r * ld + c] : 0.0; };
    auto weight = [&](int r) { return r >= 0 ? a.a[r] : 1.0; };

    int u0, i0, u1, i1, u2, i2;
    sample(0, u0, i0);
    sample(1, u1, i1);
    double p = row(a.P, a.ldp, u0), ap = row(a.AP, a.ldap, u0);
    double ei = row(a.E, a.lde, i0), aei = row(a.AE, a.ldae, i0);
    double si = 0.0, wi = 1.0;
    if constexpr (FEAT) si = row(a.S, a.lds, i0), wi = weight(i0);
    int64_t trained = 0, draws = 0;
    for (int64_t t = 0; t < maxlen; ++t) {
        sample(t + 2, u2, i2);
        const bool new_u = u1 != u0, same_i = i1 == i0;
        const double p_next = new_u ? row(a.P, a.ldp, u1) : 0.0, ap_next = new_u ? row(a.AP, a.ldap, u1) : 0.0;
        const double ei_next = same_i ? 0.0 : row(a.E, a.lde, i1), aei_next = same_i ? 0.0 : row(a.AE, a.ldae, i1);
        double si_next = 0.0, wi_next = 1.0;
        if constexpr (FEAT) si_next = row(a.S, a.lds, i1), wi_next = weight(i1);

        double qi = ei;
        if constexpr (FEAT) qi = wi * ei + si;
        const double x_pos = group_sum<W>(p * qi);
        const double bar = x_pos - 1.0;

        // the candidates: the first one with x_neg > x_pos - 1 is the violator
        bool open = u0 >= 0;
        int jv = -1, tv = 0;
        double ej = 0.0, qj = 0.0, wj = 1.0;
        const int32_t *cd = a.cand + (t0 + (open ? t : 0)) * (int64_t)D;
        for (int tb = 0; tb < D; tb += WARP_BATCH) {
            if (!__any(open)) break;                                 // wave-uniform
            int32_t j[WARP_BATCH];
            double e[WARP_BATCH], s[WARP_BATCH], w[WARP_BATCH];
#pragma unroll
            for (int x = 0; x < WARP_BATCH; ++x) j[x] = (open && tb + x < D) ? cd[tb + x] : -1;
#pragma unroll
            for (int x = 0; x < WARP_BATCH; ++x) {
                e[x] = row(a.E, a.lde, j[x]);
                s[x] = 0.0, w[x] = 1.0;
                if constexpr (FEAT) s[x] = row(a.S, a.lds, j[x]), w[x] = weight(j[x]);
            }
#pragma unroll
            for (int x = 0; x < WARP_BATCH; ++x) {
                double q = e[x];
                if constexpr (FEAT) q = w[x] * e[x] + s[x];
                const double x_neg = group_sum<W>(p * q);            // every lane of the wave
                if (open && tb + x < D) {
                    draws += 1;
                    if (j[x] >= 0 && x_neg > bar) {
                        jv = j[x], tv = tb + x, ej = e[x], qj = q, wj = w[x];
                        open = false;
                    }
                }
            }
        }

        const bool hit = jv >= 0;
        const double lw = hit ? a.table[tv] : 0.0;
        const double aej = (hit && qcol) ? a.AE[(int64_t)jv * a.ldae + c] : 1.0;
        const double g_u = lw * (qj - qi), g_j = lw * p, g_i = -g_j;
        double gi_w = g_i, gj_w = g_j;
        if constexpr (FEAT) gi_w = wi * g_i, gj_w = wj * g_j;
        const bool up = hit && pcol, uq = hit && qcol;
        const double p_new = up ? p - (a.lr / sqrt(ap)) * g_u : p, ap_new = up ? ap + g_u * g_u : ap;
        const double ei_new = uq ? ei - (a.lr / sqrt(aei)) * gi_w : ei, aei_new = uq ? aei + gi_w * gi_w : aei;
        const double ej_new = uq ? ej - (a.lr / sqrt(aej)) * gj_w : ej, aej_new = uq ? aej + gj_w * gj_w : aej;
        if (hit) {
            if (pcol) {
                a.P[(int64_t)u0 * a.ldp + c] = p_new;
                a.AP[(int64_t)u0 * a.ldap + c] = ap_new;
            }
            if (qcol) {
                a.E[(int64_t)i0 * a.lde + c] = ei_new;
                a.AE[(int64_t)i0 * a.ldae + c] = aei_new;
                a.E[(int64_t)jv * a.lde + c] = ej_new;
                a.AE[(int64_t)jv * a.ldae + c] = aej_new;
                if constexpr (FEAT) {
                    double *gi = a.G + (int64_t)i0 * a.ldg + c, *gj = a.G + (int64_t)jv * a.ldg + c;
                    *gi = *gi + g_i;
                    *gj = *gj + g_j;
                }
            }
            trained += 1;
        }
        const bool from_j = hit && i1 == jv;
        p = new_u ? p_next : p_new;
        ap = new_u ? ap_next : ap_new;
        ei = same_i ? ei_new : from_j ? ej_new : ei_next;
        aei = same_i ? aei_new : from_j ? aej_new : aei_next;
        si = si_next, wi = wi_next;
        u0 = u1, i0 = i1;
        u1 = u2, i1 = i2;
    }
    if (b < a.B && c == 0) {
        const int64_t BB = (int64_t)a.B * a.B, at = (int64_t)stratum * a.B + b;
        a.counts[at] = trained;
        a.counts[BB + at] = len - trained;
        a.counts[2 * BB + at] = draws;
    }
}

extern "C" int32_t pk_warp_max_rank(void) { return WARP_MAX_RANK; }
extern "C" int64_t pk_warp_work_bytes(int32_t blocks) { return pair_work_bytes(blocks); }

extern "C" int pk_warp_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, int64_t n_items, int64_t n_labels,
                                 int32_t max_sampled, const int64_t *block_ptr_dev, const int32_t *users_dev, const int32_t *items_dev,
                                 const int32_t *cand_dev, const double *loss_table_dev, double *P_dev, int64_t ldp, double *E_dev,
                                 int64_t lde, double *AP_dev, int64_t ldap, double *AE_dev, int64_t ldae, double learning_rate,
                                 const double *a_dev, const int64_t *row_ptr_dev, const int32_t *row_idx_dev, const double *row_val_dev,
                                 const int64_t *col_ptr_dev, const int32_t *col_idx_dev, const double *col_val_dev, double *L_dev,
                                 int64_t ldl, double *AL_dev, int64_t ldal, double *S_dev, int64_t lds, double *G_dev, int64_t ldg,
                                 void *work_dev, int64_t *counts_dev) {
    const int cols = rank + 1;
    const int rc = pk_sweep_check("pk_warp_epoch_f64", blocks, rank, WARP_MAX_RANK, cols,
                                  nnz >= 0 && n_items >= 1 && n_items < ((int64_t)1 << 31) && n_labels >= 0,
                                  block_ptr_dev && P_dev && E_dev && AP_dev && AE_dev && loss_table_dev && work_dev && counts_dev &&
                                      P_dev != E_dev && AP_dev != AE_dev && AP_dev != P_dev && AE_dev != E_dev,
                                  nnz == 0 || (users_dev && items_dev && cand_dev), "samples", ldp, lde);
    if (rc != PK_OK) return rc;
    PK_REQUIRE(max_sampled >= 1 && max_sampled <= PK_WARP_MAX_SAMPLED, "pk_warp_epoch_f64: max_sampled %d outside 1..%d", (int)max_sampled,
               PK_WARP_MAX_SAMPLED);
    PK_REQUIRE(ldap >= cols && ldae >= cols, "pk_warp_epoch_f64: bad leading dimension of the adagrad state (rank + 1 columns)");
    const bool featured = a_dev != nullptr;
    if (featured) {
        // (the index and value arrays may be NULL when no item carries a label)
        PK_REQUIRE(n_labels < ((int64_t)1 << 31) && row_ptr_dev && col_ptr_dev,
                   "pk_warp_epoch_f64: the item features need the row pointers of their CSR and the column pointers of their CSC");
        PK_REQUIRE(S_dev && G_dev && S_dev != G_dev && lds >= cols && ldg >= cols && (n_labels == 0 || (L_dev && AL_dev && L_dev != AL_dev)) &&
                       ldl >= cols && ldal >= cols,
                   "pk_warp_epoch_f64: with item features the label embeddings, their state, S and G are needed (rank + 1 columns)");
    } else {
        PK_REQUIRE(!row_ptr_dev && !col_ptr_dev && !L_dev && !AL_dev && !S_dev && !G_dev,
                   "pk_warp_epoch_f64: item features without their weights a_dev");
    }
    WarpArgs a;
    a.B = blocks, a.rank = rank, a.D = max_sampled;
    a.block_ptr = block_ptr_dev, a.users = users_dev, a.items = items_dev, a.cand = cand_dev, a.table = loss_table_dev;
    a.P = P_dev, a.E = E_dev, a.AP = AP_dev, a.AE = AE_dev, a.ldp = ldp, a.lde = lde, a.ldap = ldap, a.ldae = ldae;
    a.lr = learning_rate;
    a.a = a_dev, a.S = S_dev, a.G = G_dev, a.lds = lds, a.ldg = ldg;
    a.counts = (int64_t *)work_dev;
    WarpFeatures f = {};
    f.n_items = n_items, f.n_labels = n_labels, f.a = a_dev;
    f.row_ptr = row_ptr_dev, f.row_idx = row_idx_dev, f.row_val = row_val_dev;
    f.col_ptr = col_ptr_dev, f.col_idx = col_idx_dev, f.col_val = col_val_dev;
    f.L = L_dev, f.AL = AL_dev, f.ldl = ldl, f.ldal = ldal, f.S = S_dev, f.G = G_dev, f.lds = lds, f.ldg = ldg;
    hipStream_t st = pk_stream(stream);
    return pk_sweep_epoch(
        blocks, cols,
        [&](auto w, unsigned grid, int s) -> int {
            if (featured) {
                const int irc = warp_launch_image(st, f, cols, true);              // S for this stratum; G starts at zero
                if (irc != PK_OK) return irc;
                hipLaunchKernelGGL((warp_stratum_kernel<w(), true>), dim3(grid), dim3(WARP_THREADS), 0, st, a, s);
            } else {
                hipLaunchKernelGGL((warp_stratum_kernel<w(), false>), dim3(grid), dim3(WARP_THREADS), 0, st, a, s);
            }
            PK_CHECK_LAUNCH("warp_stratum_kernel");
            return featured ? warp_launch_label_step(st, f, cols, learning_rate) : PK_OK;
        },
        [&]() -> int {
            if (featured) {
                const int zrc = warp_launch_zero(st, f, cols);                     // G is zero when the epoch ends
                if (zrc != PK_OK) return zrc;
            }
            return pair_launch_counts(st, (int)blocks, (const int64_t *)work_dev, counts_dev);
        });
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_warp() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&warp_zero_kernel));
}
