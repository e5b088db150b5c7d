// The rating-regression factorisation model with user and item side information (polara_amd/fm.py: the reference's
// TuriFactorizationRecommender): global mean, biases, linear terms of the side features and factorised interactions, fp64, on
// PMF's conflict-free blocked schedule.  Rank k, C = k + 2 columns, so that one lane-group dot is the whole prediction: a user
// row is [factors | bias | 1], an item row [factors | 1 | bias]; the label rows of either side carry their linear weight in
// their side's bias column and 0 in the other.  A sample touches one user identity row and one item identity row; the blocks
// of a stratum share neither, so one launch sweeps them side by side, each block sequentially by one lane group.  The label
// embeddings of BOTH sides are shared between blocks and are treated as WARP's are (warp.hip): read-only during a stratum (their
// images SU = FU LU and SI = FI LI are formed by launches before it), every block adds the label gradients of its own rows into
// its own rows of GU / GI and counts the sample there, and a launch per side after the stratum sums G over every label's rows
// in ascending order and takes one step per label.  No atomics, no flags, no grid barrier: stream order is the only
// synchronisation.  The arithmetic of a sample and of a label step is spelled out in polara_hip.h.  gfx950 only (wave = 64).
#include "pk_common.h"

// every product and sum below is rounded on its own, as NumPy rounds them (the library is built with contraction on)
#pragma clang fp contract(off)

#include "blocked_sweep.h"            // after the pragma: the shared helpers are compiled without contraction too

#define FM_MAX_RANK 62              // k + 2 columns in one wave
#define FM_LABEL_BATCH 8            // rows of a label whose loads the label step issues together

// ---- the label embeddings of one side ---------------------------------------------------------------------------------------
// the features F = diag(a) one_hot of a side as CSR (rows: users or items) and CSC (columns: labels, rows ascending), and what
// they act on
struct FmLabels {
    int64_t n_rows, n_labels;
    const int64_t *row_ptr, *col_ptr;
    const int32_t *row_idx, *col_idx;
    const double *row_val, *col_val;
    double *L, *SL;                     // the label embeddings and their step state [n_labels x C]
    int64_t ldl, ldsl;
    double *S, *G;                      // the image F L [n_rows x C]; the rows' label gradients and sample counts [n_rows x (C + 1)]
    int64_t lds, ldg;
};

// S[r] = (+0.0 + v1 * L[l1]) + v2 * L[l2] + ... over row r of F in storage order, one thread per (row, column of G): column C
// has no image; with `zero_g` the thread clears its cell of G (what the stratum before left there has been consumed)
__global__ __launch_bounds__(256) void fm_image_kernel(FmLabels f, int C, bool zero_g) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= f.n_rows * (C + 1)) return;
    const int64_t r = x / (C + 1);
    const int c = (int)(x - r * (C + 1));
    if (c < C) {
        double acc = 0.0;
        for (int64_t e = f.row_ptr[r]; e < f.row_ptr[r + 1]; ++e) acc = acc + f.row_val[e] * f.L[(int64_t)f.row_idx[e] * f.ldl + c];
        f.S[r * f.lds + c] = acc;
    }
    if (zero_g) f.G[r * f.ldg + c] = 0.0;
}

// One thread per (label, column): g = (+0.0 + v1 * G[r1]) + v2 * G[r2] + ... and N = (+0.0 + G[r1][C]) + G[r2][C] + ... over
// column l of F (rows ascending); a label none of whose rows was sampled (N == 0) takes no step; else g <- g + (lambda * N) * x
// and one adjusted step.  Columns that are never stepped leave at once: the other side's bias column, and the factor columns
// when the side data is not factorised.  G is only read here: rows carry several labels.
template <int ADJ>
__global__ __launch_bounds__(256) void fm_label_step_kernel(FmLabels f, PmfArgs a, int bias_col, bool factors, double lam_f,
                                                            double lam_lin) {
    const int k = a.rank, C = k + 2;
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= f.n_labels * C) return;
    const int64_t l = x / C;
    const int c = (int)(x - l * C);
    if (!((factors && c < k) || c == bias_col)) return;
    double g = 0.0, N = 0.0;
    const int64_t hi = f.col_ptr[l + 1];
    int64_t e = f.col_ptr[l];
    // the loads of FM_LABEL_BATCH rows are issued together, the sums stay in row order: a popular label has thousands of rows,
    // and one dependent index-then-row load per addition is what a stratum's label step then costs
    for (; e + FM_LABEL_BATCH <= hi; e += FM_LABEL_BATCH) {
        double v[FM_LABEL_BATCH], x[FM_LABEL_BATCH], n[FM_LABEL_BATCH];
#pragma unroll
        for (int j = 0; j < FM_LABEL_BATCH; ++j) {
            const double *row = f.G + (int64_t)f.col_idx[e + j] * f.ldg;
            v[j] = f.col_val[e + j], x[j] = row[c], n[j] = row[C];
        }
#pragma unroll
        for (int j = 0; j < FM_LABEL_BATCH; ++j) {
            g = g + v[j] * x[j];
            N = N + n[j];
        }
    }
    for (; e < hi; ++e) {
        const double *row = f.G + (int64_t)f.col_idx[e] * f.ldg;
        g = g + f.col_val[e] * row[c];
        N = N + row[C];
    }
    if (N == 0.0) return;
    const double x0 = f.L[l * f.ldl + c];
    g = g + ((c < k ? lam_f : lam_lin) * N) * x0;
    double s = 0.0;
    if constexpr (ADJ != PK_PMF_ADJUST_NONE) s = f.SL[l * f.ldsl + c];
    const double step = pmf_adjust<ADJ>(g, s, a);
    f.L[l * f.ldl + c] = x0 - a.eta * step;
    if constexpr (ADJ != PK_PMF_ADJUST_NONE) f.SL[l * f.ldsl + c] = s;
}

__global__ __launch_bounds__(256) void fm_zero_kernel(int64_t n, int cols, double *__restrict__ G, int64_t ldg) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n * cols) return;
    const int64_t r = x / cols;
    G[r * ldg + (x - r * cols)] = 0.0;
}

static unsigned fm_cells_grid(int64_t rows, int cols) { return (unsigned)pk_ceil_div(rows * cols > 0 ? rows * cols : 1, 256); }

static int fm_launch_image(hipStream_t st, const FmLabels &f, int C, bool zero_g) {
    hipLaunchKernelGGL(fm_image_kernel, dim3(fm_cells_grid(f.n_rows, C + 1)), dim3(256), 0, st, f, C, zero_g);
    PK_CHECK_LAUNCH("fm_image_kernel");
    return PK_OK;
}

static int fm_launch_label_step(hipStream_t st, const FmLabels &f, const PmfArgs &a, int adjust, int bias_col, bool factors,
                                double lam_f, double lam_lin) {
    if (f.n_labels == 0) return PK_OK;
    const dim3 grid(fm_cells_grid(f.n_labels, a.rank + 2));
    if (adjust == PK_PMF_ADJUST_NONE)
        hipLaunchKernelGGL((fm_label_step_kernel<PK_PMF_ADJUST_NONE>), grid, dim3(256), 0, st, f, a, bias_col, factors, lam_f, lam_lin);
    else if (adjust == PK_PMF_ADJUST_ADAGRAD)
        hipLaunchKernelGGL((fm_label_step_kernel<PK_PMF_ADJUST_ADAGRAD>), grid, dim3(256), 0, st, f, a, bias_col, factors, lam_f, lam_lin);
    else
        hipLaunchKernelGGL((fm_label_step_kernel<PK_PMF_ADJUST_RMSPROP>), grid, dim3(256), 0, st, f, a, bias_col, factors, lam_f, lam_lin);
    PK_CHECK_LAUNCH("fm_label_step_kernel");
    return PK_OK;
}

static int fm_launch_zero(hipStream_t st, const FmLabels &f, int C) {
    hipLaunchKernelGGL(fm_zero_kernel, dim3(fm_cells_grid(f.n_rows, C + 1)), dim3(256), 0, st, f.n_rows, C + 1, f.G, f.ldg);
    PK_CHECK_LAUNCH("fm_zero_kernel");
    return PK_OK;
}

// ---- the sweep --------------------------------------------------------------------------------------------------------------
// what a block reads and writes of one side's features: the rows' weights, the image, and its own rows of G
struct FmSide {
    const double *a, *S;
    double *G;
    int64_t lds, ldg;
};

// pmf: the schedule, P, Q = the item identity rows E, both step states, eta, the adjuster's constants and the block sums
struct FmArgs {
    PmfArgs pmf;
    double mu, lam_f, lam_lin;
    FmSide u, i;
};

// W lanes per block, 64 / W blocks per wave; lane c holds column c of the k + 2.  The loop runs to the longest block of the wave
// with every lane active (the butterfly reads its neighbours); a group past the end of its block computes on zeros and stores
// nothing.  Sample t + 1's rows — P, E, their step state and, with features, the rows of G with their counts — are loaded while
// sample t is computed, unless they are sample t's own rows, whose new values then stay in registers, as in
// pmf_stratum_kernel.  The images and the weights are read-only here.  FU / FI: the side has features.
template <int W, int ADJ, bool FU, bool FI>
__global__ __launch_bounds__(PMF_THREADS) void fm_stratum_kernel(FmArgs args, int stratum) {
    const PmfArgs &a = args.pmf;
    int c;
    const int64_t b = pk_sweep_lanes<W>(c);
    const int k = a.rank, C = k + 2;
    const bool col = c < C;
    const bool up = c <= k, uq = c < k || c == k + 1;           // the columns of a user row / an item row that are stepped
    const double lam = c < k ? args.lam_f : args.lam_lin;
    int64_t t0, len;
    const int64_t maxlen = pk_sweep_range<W>(a.B, a.block_ptr, stratum, b, t0, len);

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
    auto weight = [&](const double *w, int r) { return r >= 0 ? w[r] : 1.0; };
    auto count = [&](const double *G, int64_t ld, int r) { return r >= 0 ? G[(int64_t)r * ld + C] : 0.0; };

    int m0, n0, m1, n1, m2, n2;
    double v0, v1, v2;
    sample(0, m0, n0, v0);
    sample(1, m1, n1, v1);
    double p = row(a.P, a.ldp, m0), e = row(a.Q, a.ldq, n0);
    double sp = ADJ ? row(a.SP, a.ldsp, m0) : 0.0, se = ADJ ? row(a.SQ, a.ldsq, n0) : 0.0;
    double su = 0.0, au = 1.0, gu = 0.0, nu = 0.0, si = 0.0, ai = 1.0, gi = 0.0, ni = 0.0;
    if constexpr (FU) {
        su = row(args.u.S, args.u.lds, m0), au = weight(args.u.a, m0);
        gu = row(args.u.G, args.u.ldg, m0), nu = count(args.u.G, args.u.ldg, m0);
    }
    if constexpr (FI) {
        si = row(args.i.S, args.i.lds, n0), ai = weight(args.i.a, n0);
        gi = row(args.i.G, args.i.ldg, n0), ni = count(args.i.G, args.i.ldg, n0);
    }
    double sse = 0.0;
    for (int64_t t = 0; t < maxlen; ++t) {
        sample(t + 2, m2, n2, v2);
        const bool new_m = m1 != m0, new_n = n1 != n0;
        const double p_next = new_m ? row(a.P, a.ldp, m1) : 0.0, e_next = new_n ? row(a.Q, a.ldq, n1) : 0.0;
        const double sp_next = (ADJ && new_m) ? row(a.SP, a.ldsp, m1) : 0.0, se_next = (ADJ && new_n) ? row(a.SQ, a.ldsq, n1) : 0.0;
        double su_next = 0.0, au_next = 1.0, gu_next = 0.0, nu_next = 0.0, si_next = 0.0, ai_next = 1.0, gi_next = 0.0, ni_next = 0.0;
        if constexpr (FU) {
            su_next = row(args.u.S, args.u.lds, m1), au_next = weight(args.u.a, m1);
            if (new_m) gu_next = row(args.u.G, args.u.ldg, m1), nu_next = count(args.u.G, args.u.ldg, m1);
        }
        if constexpr (FI) {
            si_next = row(args.i.S, args.i.lds, n1), ai_next = weight(args.i.a, n1);
            if (new_n) gi_next = row(args.i.G, args.i.ldg, n1), ni_next = count(args.i.G, args.i.ldg, n1);
        }

        double pt = p, qt = e;
        if constexpr (FU) pt = au * p + su;
        if constexpr (FI) qt = ai * e + si;
        const double dot = group_sum<W>(pt * qt);
        const double err = (args.mu + dot) - v0;
        const double eq = err * qt, ep = err * pt;              // what the user side / the item side receives
        double gp = eq, gq = ep;
        if constexpr (FU) gp = au * eq;
        if constexpr (FI) gq = ai * ep;
        gp = gp + lam * p;
        gq = gq + lam * e;
        double sp_new = sp, se_new = se;
        const double ap = pmf_adjust<ADJ>(gp, sp_new, a);
        const double aq = pmf_adjust<ADJ>(gq, se_new, a);
        const double p_new = up ? p - a.eta * ap : p;
        const double e_new = uq ? e - a.eta * aq : e;
        if constexpr (ADJ != PK_PMF_ADJUST_NONE) {
            sp = up ? sp_new : sp;
            se = uq ? se_new : se;
        }
        const double gu_new = gu + eq, nu_new = nu + 1.0, gi_new = gi + ep, ni_new = ni + 1.0;
        if (m0 >= 0) {
            if (col) {
                if (up) {
                    a.P[(int64_t)m0 * a.ldp + c] = p_new;
                    if constexpr (ADJ != PK_PMF_ADJUST_NONE) a.SP[(int64_t)m0 * a.ldsp + c] = sp;
                }
                if (uq) {
                    a.Q[(int64_t)n0 * a.ldq + c] = e_new;
                    if constexpr (ADJ != PK_PMF_ADJUST_NONE) a.SQ[(int64_t)n0 * a.ldsq + c] = se;
                }
                if constexpr (FU) args.u.G[(int64_t)m0 * args.u.ldg + c] = gu_new;
                if constexpr (FI) args.i.G[(int64_t)n0 * args.i.ldg + c] = gi_new;
            }
            if (c == 0) {
                if constexpr (FU) args.u.G[(int64_t)m0 * args.u.ldg + C] = nu_new;
                if constexpr (FI) args.i.G[(int64_t)n0 * args.i.ldg + C] = ni_new;
            }
            sse = sse + err * err;
        }
        p = new_m ? p_next : p_new;
        e = new_n ? e_next : e_new;
        if constexpr (ADJ != PK_PMF_ADJUST_NONE) {
            sp = new_m ? sp_next : sp;
            se = new_n ? se_next : se;
        }
        if constexpr (FU) su = su_next, au = au_next, gu = new_m ? gu_next : gu_new, nu = new_m ? nu_next : nu_new;
        if constexpr (FI) si = si_next, ai = ai_next, gi = new_n ? gi_next : gi_new, ni = new_n ? ni_next : ni_new;
        m0 = m1, n0 = n1, v0 = v1;
        m1 = m2, n1 = n2, v1 = v2;
    }
    if (b < a.B && c == 0) a.block_sse[(int64_t)stratum * a.B + b] = sse;
}

// the instance of fm_stratum_kernel for the adjuster code, on `st`
template <int W, bool FU, bool FI>
static int fm_launch(hipStream_t st, int adjust, unsigned grid, const FmArgs &a, int stratum) {
    if (adjust == PK_PMF_ADJUST_NONE)
        hipLaunchKernelGGL((fm_stratum_kernel<W, PK_PMF_ADJUST_NONE, FU, FI>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
    else if (adjust == PK_PMF_ADJUST_ADAGRAD)
        hipLaunchKernelGGL((fm_stratum_kernel<W, PK_PMF_ADJUST_ADAGRAD, FU, FI>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
    else
        hipLaunchKernelGGL((fm_stratum_kernel<W, PK_PMF_ADJUST_RMSPROP, FU, FI>), dim3(grid), dim3(PMF_THREADS), 0, st, a, stratum);
    PK_CHECK_LAUNCH("fm_stratum_kernel");
    return PK_OK;
}

// ---- the entries ------------------------------------------------------------------------------------------------------------
extern "C" int32_t pk_fm_max_rank(void) { return FM_MAX_RANK; }

static int fm_check_rank(const char *entry, int rank) {
    PK_REQUIRE(rank >= 1 && rank <= FM_MAX_RANK, "%s: rank %d outside 1..%d", entry, rank, FM_MAX_RANK);
    return PK_OK;
}

static int fm_check_adjust(const char *entry, int adjust) {
    PK_REQUIRE(adjust == PK_PMF_ADJUST_NONE || adjust == PK_PMF_ADJUST_ADAGRAD || adjust == PK_PMF_ADJUST_RMSPROP,
               "%s: unknown gradient adjustment %d", entry, adjust);
    return PK_OK;
}

static PmfArgs fm_step_constants(int rank, double eta, double gamma, double smoothing) {
    PmfArgs a = {};
    a.rank = rank;
    a.eta = eta;
    a.gamma = gamma, a.one_minus_gamma = 1.0 - gamma, a.smoothing = smoothing;
    return a;
}

extern "C" int pk_fm_label_image_f64(void *stream, int32_t rank, int64_t n_rows, int64_t n_labels, const int64_t *row_ptr_dev,
                                     const int32_t *row_idx_dev, const double *row_val_dev, const double *L_dev, int64_t ldl,
                                     double *S_dev, int64_t lds) {
    const int rc = fm_check_rank("pk_fm_label_image_f64", rank);
    if (rc != PK_OK) return rc;
    const int C = rank + 2;
    PK_REQUIRE(n_rows >= 1 && n_rows < ((int64_t)1 << 31) && n_labels >= 0 && n_labels < ((int64_t)1 << 31) && row_ptr_dev && S_dev &&
                   (n_labels == 0 || L_dev) && ldl >= C && lds >= C,
               "pk_fm_label_image_f64: bad arguments");
    FmLabels f = {};
    f.n_rows = n_rows, f.n_labels = n_labels;
    f.row_ptr = row_ptr_dev, f.row_idx = row_idx_dev, f.row_val = row_val_dev;
    f.L = const_cast<double *>(L_dev), f.ldl = ldl, f.S = S_dev, f.lds = lds;
    return fm_launch_image(pk_stream(stream), f, C, false);
}

extern "C" int pk_fm_label_step_f64(void *stream, int32_t rank, int32_t item_side, int32_t label_factors, int64_t n_rows,
                                    int64_t n_labels, const int64_t *col_ptr_dev, const int32_t *col_idx_dev,
                                    const double *col_val_dev, double *G_dev, int64_t ldg, double *L_dev, int64_t ldl,
                                    double *SL_dev, int64_t ldsl, double step, double regularization, double linear_regularization,
                                    int32_t adjust, double gamma, double smoothing) {
    int rc = fm_check_rank("pk_fm_label_step_f64", rank);
    if (rc == PK_OK) rc = fm_check_adjust("pk_fm_label_step_f64", adjust);
    if (rc != PK_OK) return rc;
    const int C = rank + 2;
    PK_REQUIRE(n_rows >= 1 && n_rows < ((int64_t)1 << 31) && n_labels >= 0 && n_labels < ((int64_t)1 << 31) && col_ptr_dev && G_dev &&
                   (n_labels == 0 || (L_dev && (adjust == PK_PMF_ADJUST_NONE || (SL_dev && SL_dev != L_dev && ldsl >= C)))) &&
                   ldg >= C + 1 && ldl >= C,
               "pk_fm_label_step_f64: bad arguments");
    FmLabels f = {};
    f.n_rows = n_rows, f.n_labels = n_labels;
    f.col_ptr = col_ptr_dev, f.col_idx = col_idx_dev, f.col_val = col_val_dev;
    f.L = L_dev, f.SL = SL_dev, f.ldl = ldl, f.ldsl = ldsl, f.G = G_dev, f.ldg = ldg;
    hipStream_t st = pk_stream(stream);
    rc = fm_launch_label_step(st, f, fm_step_constants(rank, step, gamma, smoothing), adjust, item_side ? rank + 1 : rank,
                              label_factors != 0, regularization, linear_regularization);
    return rc != PK_OK ? rc : fm_launch_zero(st, f, C);
}

// one side's features as the entry receives them: checked and packed; `a_dev == NULL`: the side has none
static int fm_side(const char *side, int C, int adjust, int64_t n_rows, int64_t n_labels, const double *a_dev,
                   const int64_t *row_ptr_dev, const int32_t *row_idx_dev, const double *row_val_dev, const int64_t *col_ptr_dev,
                   const int32_t *col_idx_dev, const double *col_val_dev, double *L_dev, int64_t ldl, double *SL_dev, int64_t ldsl,
                   double *S_dev, int64_t lds, double *G_dev, int64_t ldg, FmLabels &f, FmSide &s) {
    f = FmLabels();
    s = FmSide();
    if (!a_dev) {
        PK_REQUIRE(!row_ptr_dev && !col_ptr_dev && !L_dev && !SL_dev && !S_dev && !G_dev,
                   "pk_fm_epoch_f64: %s features without their weights", side);
        return PK_OK;
    }
    // (the index and value arrays may be NULL when no row carries a label)
    PK_REQUIRE(n_labels >= 0 && n_labels < ((int64_t)1 << 31) && row_ptr_dev && col_ptr_dev,
               "pk_fm_epoch_f64: the %s features need the row pointers of their CSR and the column pointers of their CSC", side);
    PK_REQUIRE(S_dev && G_dev && S_dev != G_dev && lds >= C && ldg >= C + 1 &&
                   (n_labels == 0 || (L_dev && ldl >= C && (adjust == PK_PMF_ADJUST_NONE || (SL_dev && SL_dev != L_dev && ldsl >= C)))),
               "pk_fm_epoch_f64: with %s features the label embeddings, their state, S (rank + 2 columns) and G (rank + 3) are needed",
               side);
    f.n_rows = n_rows, f.n_labels = n_labels;
    f.row_ptr = row_ptr_dev, f.row_idx = row_idx_dev, f.row_val = row_val_dev;
    f.col_ptr = col_ptr_dev, f.col_idx = col_idx_dev, f.col_val = col_val_dev;
    f.L = L_dev, f.SL = SL_dev, f.ldl = ldl, f.ldsl = ldsl, f.S = S_dev, f.G = G_dev, f.lds = lds, f.ldg = ldg;
    s.a = a_dev, s.S = S_dev, s.G = G_dev, s.lds = lds, s.ldg = ldg;
    return PK_OK;
}

extern "C" int pk_fm_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, int64_t n_users, int64_t n_items,
                               const int64_t *block_ptr_dev, const int32_t *users_dev, const int32_t *items_dev, const double *vals_dev,
                               double mean, double *P_dev, int64_t ldp, double *E_dev, int64_t lde, double step, double regularization,
                               double linear_regularization, int32_t adjust, double *SP_dev, int64_t ldsp, double *SE_dev,
                               int64_t ldse, double gamma, double smoothing, int32_t label_factors,
                               int64_t n_ulabels, const double *au_dev, const int64_t *urow_ptr_dev, const int32_t *urow_idx_dev,
                               const double *urow_val_dev, const int64_t *ucol_ptr_dev, const int32_t *ucol_idx_dev,
                               const double *ucol_val_dev, double *LU_dev, int64_t ldlu, double *SLU_dev, int64_t ldslu, double *SU_dev,
                               int64_t ldsu, double *GU_dev, int64_t ldgu,
                               int64_t n_ilabels, const double *ai_dev, const int64_t *irow_ptr_dev, const int32_t *irow_idx_dev,
                               const double *irow_val_dev, const int64_t *icol_ptr_dev, const int32_t *icol_idx_dev,
                               const double *icol_val_dev, double *LI_dev, int64_t ldli, double *SLI_dev, int64_t ldsli, double *SI_dev,
                               int64_t ldsi, double *GI_dev, int64_t ldgi, double *work_dev, double *sse_dev) {
    const int C = rank + 2;
    int rc = pk_sweep_check("pk_fm_epoch_f64", blocks, rank, FM_MAX_RANK, C,
                            nnz >= 0 && n_users >= 1 && n_users < ((int64_t)1 << 31) && n_items >= 1 && n_items < ((int64_t)1 << 31),
                            block_ptr_dev && P_dev && E_dev && work_dev && sse_dev && P_dev != E_dev,
                            nnz == 0 || (users_dev && items_dev && vals_dev), "interactions", ldp, lde, adjust, SP_dev, SE_dev, ldsp, ldse);
    if (rc != PK_OK) return rc;
    PK_REQUIRE(adjust == PK_PMF_ADJUST_NONE || (ldsp >= C && ldse >= C && SP_dev != P_dev && SE_dev != E_dev),
               "pk_fm_epoch_f64: bad leading dimension of the step state (rank + 2 columns)");
    FmArgs a = {};
    FmLabels fu, fi;
    rc = fm_side("user", C, adjust, n_users, n_ulabels, au_dev, urow_ptr_dev, urow_idx_dev, urow_val_dev, ucol_ptr_dev, ucol_idx_dev,
                 ucol_val_dev, LU_dev, ldlu, SLU_dev, ldslu, SU_dev, ldsu, GU_dev, ldgu, fu, a.u);
    if (rc != PK_OK) return rc;
    rc = fm_side("item", C, adjust, n_items, n_ilabels, ai_dev, irow_ptr_dev, irow_idx_dev, irow_val_dev, icol_ptr_dev, icol_idx_dev,
                 icol_val_dev, LI_dev, ldli, SLI_dev, ldsli, SI_dev, ldsi, GI_dev, ldgi, fi, a.i);
    if (rc != PK_OK) return rc;
    a.pmf = fm_step_constants(rank, step, gamma, smoothing);
    a.pmf.B = blocks;
    a.pmf.block_ptr = block_ptr_dev, a.pmf.users = users_dev, a.pmf.items = items_dev, a.pmf.vals = vals_dev;
    a.pmf.P = P_dev, a.pmf.Q = E_dev, a.pmf.ldp = ldp, a.pmf.ldq = lde;
    a.pmf.SP = SP_dev, a.pmf.SQ = SE_dev, a.pmf.ldsp = ldsp, a.pmf.ldsq = ldse;
    a.pmf.block_sse = work_dev;
    a.mu = mean, a.lam_f = regularization, a.lam_lin = linear_regularization;
    const bool with_u = au_dev != nullptr, with_i = ai_dev != nullptr, factors = label_factors != 0;
    hipStream_t st = pk_stream(stream);
    return pk_sweep_epoch(
        blocks, C,
        [&](auto w, unsigned grid, int s) -> int {
            int src = PK_OK;
            if (with_u) src = fm_launch_image(st, fu, C, true);                     // SU for this stratum; GU starts at zero
            if (src == PK_OK && with_i) src = fm_launch_image(st, fi, C, true);
            if (src != PK_OK) return src;
            src = with_u ? (with_i ? fm_launch<w(), true, true>(st, adjust, grid, a, s) : fm_launch<w(), true, false>(st, adjust, grid, a, s))
                         : (with_i ? fm_launch<w(), false, true>(st, adjust, grid, a, s) : fm_launch<w(), false, false>(st, adjust, grid, a, s));
            if (src == PK_OK && with_u) src = fm_launch_label_step(st, fu, a.pmf, adjust, rank, factors, regularization, linear_regularization);
            if (src == PK_OK && with_i) src = fm_launch_label_step(st, fi, a.pmf, adjust, rank + 1, factors, regularization, linear_regularization);
            return src;
        },
        [&]() -> int {
            int erc = PK_OK;
            if (with_u) erc = fm_launch_zero(st, fu, C);                            // G is zero when the epoch ends
            if (erc == PK_OK && with_i) erc = fm_launch_zero(st, fi, C);
            return erc != PK_OK ? erc : pmf_launch_sse(st, (int)blocks, work_dev, sse_dev);
        });
}

// eager load of this translation unit's code object (pk_warm_up, api.cpp)
hipError_t pk_tu_load_fm() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&fm_zero_kernel));
}
