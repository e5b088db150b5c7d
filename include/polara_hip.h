/*
 * polara_hip.h — C ABI of libpolarahip.so: hand-written HIP kernels (gfx950 / MI355X) for the
 * factorization-and-scoring hot path of evfro/polara (PureSVD + CoFFee).
 *
 * The reference is pure Python and has NO FFI of its own; each entry point below replaces one
 * NumPy/SciPy/numba call site on the hot path (cited as file:line relative to the reference
 * tree).  INTEGRATION.md shows the ctypes binding a Polara maintainer would add.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.
 *  - All `*_dev` pointers are DEVICE pointers (HBM) owned by the caller (the host layer allocates
 *    them through torch, cupy, hipMalloc — anything).  The library never allocates device memory
 *    and keeps no global state; scratch space is passed explicitly (`work`, sized by the matching
 *    pk_*_work_bytes function).
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every call only ENQUEUES
 *    work on that stream and returns; the caller synchronises.
 *  - Return value: 0 = ok, negative = error class (PK_E_*).  pk_last_error() returns a
 *    thread-local message for the last failing call on the calling thread.
 *  - Matrices are row-major with an explicit leading dimension (in elements).
 *  - Index dtypes: row pointers int64, column indices int32, results int64 (like the reference's
 *    `top_recs`, models.py:400).
 */
#ifndef POLARA_HIP_H
#define POLARA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PK_OK 0
#define PK_E_INVALID (-1)  /* bad argument                                  */
#define PK_E_LAUNCH (-2)   /* HIP launch / runtime error                    */
#define PK_E_UNSUPPORTED (-3)
#define PK_E_NOCONV (-4)   /* pk_svd_build: stopped at max_outer without converging (ARPACK's ArpackNoConvergence) */

#define PK_VAL_F32 0
#define PK_VAL_F64 1

const char *pk_last_error(void);
int pk_version(void);
/* Process-wide options, set by explicit calls — the library reads NO environment variable (round 6).  They exist for the
 * tests, which force a code path on inputs too small to take it by themselves:
 *   "score_boot_tiles"     tiles of the sweep's threshold bootstrap (default 16; 0 = off)
 *   "score_head_tiles"     head of the two-phase sweep whatever the user count (default: pk_score_two_phase_plan's rule; 0 = off)
 *   "score_phase2_splits"  item splits of its second phase
 *   "slim_r_global"        pk_slim_solve_f64 keeps the residual rows in HBM at every n (default 0: only beyond pk_slim_lds_items())
 * unset != 0 returns the option to its default.  Unknown names: PK_E_INVALID. */
int pk_set_option(const char *name, int32_t value, int32_t unset);
/* hipMemcpyAsync device -> host on `stream` (pinned destination: asynchronous): the hand-over of a pass's lists as one more
 * call of the pass (the reference returns host arrays: models.py:400-405). */
int pk_copy_to_host_async(void *stream, void *dst_host, const void *src_dev, int64_t bytes);
/* number of visible HIP devices (>=1 required by every compute call); fills name of `device`. */
int pk_device_info(int device, char *name, int name_len, int *cu_count, int64_t *hbm_bytes);
/* Loads every code object of the library on the current device (the runtime would otherwise load each translation
 * unit's at the first launch of one of its kernels — inside the caller's first build).  Called by pk_ctx_create and by
 * the Python layer's HipOps(); idempotent, a few milliseconds once per process and device. */
int pk_warm_up(void);

/* ------------------------------------------------------------------------------------------
 * K1 / K4.  CSR x dense  (fp64 accumulate):   out[r, 0:nc] = sum_p vals[p] * X[indices[p], 0:nc]
 *
 * Replaces: scipy `csr_matvec(s)` inside ARPACK's reverse-communication loop for
 * `svds(A, k)` (models.py:841-844: operator XH_X = A^T(A x)), and `test_matrix.dot(v)`
 * (models.py:860, fold-in E = A_test V).  A^T products use the same kernel on the CSC arrays.
 *
 * Work is described by a task list built once per matrix by the host layer (polara_amd/csr.py):
 * task t covers nnz range [task_begin[t], task_end[t]) of row task_row[t]; rows longer than the
 * split threshold are cut into several tasks whose partial sums go to `partial[task_slot[t]]`
 * (task_slot >= 0) and are added in slot order by a fix-up pass (deterministic, no atomics).
 * ------------------------------------------------------------------------------------------ */
/* The plain product, one entry.  The dense block X is fp64 (x_kind = PK_VAL_F64) or fp32 (PK_VAL_F32; needs nc % 4 == 0,
 * ldx % 4 == 0 and a 16-byte aligned X, else PK_E_UNSUPPORTED); accumulation and output are fp64.  The fp32 block serves
 * the approximate fold-in of the scoring pass: E' = A_test fl32(V) moves half the gather bytes of models.py:860's left
 * factor; the re-scoring kernel certifies the result against the rounding of V (pk_rescore_f64).
 * Task rows are numbered from `row_base` (task t writes output row task_row[t] - row_base — a row block of a larger plan
 * runs as its own launch; a row base needs accumulate), and with accumulate != 0 the result is ADDED to out; the whole
 * product of a matrix is row_base = 0, accumulate = 0.  Used for the transposed product of the build, Z = A^T Y
 * (models.py:844's rmatvec), cut into user blocks: the CSC of every block is one slice of a (block, item)-ordered plan
 * (pk_csr_transpose with rows_per_block > 0), block b adds its share to Z in launch order (deterministic), and the rows
 * of Y that one launch gathers stay cache-resident instead of spanning the whole user range.
 * EVERY row of X must be finite, rows that no entry references included: a task is processed in steps of several
 * entries, and the padded steps of its last chunk multiply row 0 of X by a zero weight instead of branching
 * (0 * inf = NaN would reach the sum).  X must therefore have at least one row whenever there are tasks.
 * Every argument rule is checked before anything is launched, for n_tasks = 0 too. */
int pk_spmm_csr_ex(void *stream,
                   int64_t n_tasks, const int32_t *task_row_dev, const int64_t *task_begin_dev,
                   const int64_t *task_end_dev, const int32_t *task_slot_dev,
                   int64_t n_long, const int32_t *long_row_dev, const int32_t *long_slot_begin_dev,
                   const int32_t *long_slot_end_dev,
                   const int32_t *indices_dev, const void *vals_dev, int val_kind,
                   const void *X_dev, int x_kind, int64_t ldx, int32_t nc,
                   double *out_dev, int64_t ldo, double *partial_dev /* [n_slots x nc] or NULL */,
                   int64_t row_base, int32_t accumulate,
                   int64_t x_rows /* rows of X (= columns of the sparse matrix), or 0 if unknown: with fewer than 2^24 rows
                   and X below 4 GiB the kernels address X with 32-bit offsets (a quarter of the address arithmetic) */);

/* ------------------------------------------------------------------------------------------
 * Ingest.  The index work around the hot path, on the device:
 * `coo_matrix((val, (rows, cols))).tocsr()` of get_training_matrix / get_test_matrix
 * (models.py:172-175, 198-203 <- data.py:794-817, 835-862: duplicates summed, rows sorted by column),
 * the CSC image behind the transposed products of `svds` (models.py:844), and the wave-task plans.
 * Building blocks: a stable LSD radix sort of (key, u32 payload) pairs and an exclusive scan.
 * ------------------------------------------------------------------------------------------ */
/* out[0..n] = exclusive prefix sums of in[0..n-1] (out[n] = total).  work >= pk_scan_work_bytes(n). */
int64_t pk_scan_work_bytes(int64_t n);
int pk_exclusive_scan_i32(void *stream, int64_t n, const int32_t *in_dev, int64_t *out_dev, void *work_dev);
/* Stable ascending sort of n (key, payload) pairs by the low key_bits bits of the key (key_bytes = 4 or 8).
 * The sorted pairs end in (keys, vals) when *result_in_tmp == 0, else in (keys_tmp, vals_tmp).
 * work >= pk_radix_work_bytes(n). */
int64_t pk_radix_work_bytes(int64_t n);
int pk_radix_sort_pairs(void *stream, int64_t n, int32_t key_bytes, void *keys_dev, uint32_t *vals_dev,
                        void *keys_tmp_dev, uint32_t *vals_tmp_dev, int32_t key_bits, void *work_dev,
                        int32_t *result_in_tmp);
/* The serving order of the catalogue: rows of V [n x K] by DESCENDING Euclidean norm, ties by row id (the order of
 * `np.argsort(-np.linalg.norm(V, axis=1), kind='stable')`; the reference keeps V as built, models.py:849 — the re-indexing
 * serves the sweep's pruning bound).  order_dev[p] = the row at position p, rank_dev[row] = its position, V_sorted_dev (or
 * NULL) [n x K] = the rows in that order.  work >= pk_row_norm_order_work_bytes(n). */
int64_t pk_row_norm_order_work_bytes(int64_t n);
int pk_row_norm_order_f64(void *stream, int64_t n, int32_t K, const double *V_dev, int64_t ldv, int32_t *order_dev,
                          int32_t *rank_dev, double *V_sorted_dev, void *work_dev);
/* COO triplets (device arrays, any order, duplicates allowed; entry i has row rows_dev[i * idx_stride] and column
 * cols_dev[i * idx_stride] — idx_stride = 2 reads the interleaved int64 [nnz x 2] index array of `to_coo`,
 * data.py:794-817, as it is) -> canonical CSR: indptr int64[n_rows + 1],
 * indices int32 / values (val_kind) sized for nnz entries, of which the first *n_unique_dev are used (duplicates
 * are summed in their original order).  err_dev[0] != 0 afterwards = an index was out of range.
 * work >= pk_coo_to_csr_work_bytes(nnz). */
int64_t pk_coo_to_csr_work_bytes(int64_t nnz);
int pk_coo_to_csr(void *stream, int64_t nnz, const int64_t *rows_dev, const int64_t *cols_dev, int64_t idx_stride,
                  const void *vals_dev,
                  int val_kind, int64_t n_rows, int64_t n_cols, int64_t *indptr_dev, int32_t *indices_dev,
                  void *values_dev, int64_t *n_unique_dev, int32_t *err_dev, void *work_dev);
/* CSR -> CSC.  rows_per_block = 0: t_indptr int64[n_cols + 1].  rows_per_block > 0: the rows are cut into
 * ceil(n_rows / rows_per_block) blocks and t_indptr has n_blocks * n_cols + 1 entries — entry b * n_cols + c starts
 * column c restricted to the rows of block b (row ids stay global, ascending within a column segment). */
int64_t pk_csr_transpose_work_bytes(int64_t nnz);
int pk_csr_transpose(void *stream, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *indptr_dev,
                     const int32_t *indices_dev, const void *values_dev, int val_kind, int64_t rows_per_block,
                     int64_t *t_indptr_dev, int32_t *t_indices_dev, void *t_values_dev, void *work_dev);
/* Column renaming j -> col_map[j] with every row re-sorted by the new ids (row pointers unchanged). */
int64_t pk_csr_relabel_work_bytes(int64_t nnz);
int pk_csr_relabel_sorted(void *stream, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *indptr_dev,
                          const int32_t *indices_dev, const void *values_dev, int val_kind, const int32_t *col_map_dev,
                          int32_t *indices_out_dev, void *values_out_dev, void *work_dev);
/* The rows of a CSR ordered by DESCENDING stored-entry count (stable: ties by row id): perm_out[r] = the input row that
 * becomes row r.  The scoring pass groups 32 consecutive users per wave and a group sweeps the catalogue until its LAST
 * user is done; users of similar activity finish at similar depths (ML-20M-shaped: 12.3 -> 9.5 % of the tiles scored). */
int64_t pk_csr_rows_by_length_work_bytes(int64_t n_rows);
int pk_csr_rows_by_length(void *stream, int64_t n_rows, int64_t nnz, const int64_t *indptr_dev, const int32_t *indices_dev,
                          const void *values_dev, int val_kind, int32_t *perm_out_dev, int64_t *new_indptr_dev,
                          int32_t *indices_out_dev, void *values_out_dev, void *work_dev);
/* counts[k] = number of keys equal to k (item popularity: the internal item order of the device path) */
int pk_count_i32(void *stream, int64_t n, const int32_t *keys_dev, int64_t n_bins, int32_t *counts_dev);
/* Splitting raw interactions into training / testset / holdout (csrc/split.hip; `RecommenderData.prepare()`,
 * data.py:232-252, 388-458, 718-774).
 * pk_split_keys: the selection key of n candidate rows, smaller = taken first.  mode is a sum of
 *   PK_SPLIT_ASCENDING (1): key_hi ascends with the order value (else it descends: the largest values first);
 *   PK_SPLIT_RANDOM_LO (2): key_lo = mix64(mix64(seed) + pos) (else ~pos: among equal values the LAST row first, the
 *                           `keep='last'` of nlargest / nsmallest, data.py:741-746);
 *   PK_SPLIT_NO_ORDER (4):  key_hi = 0 (order_vals_dev may be NULL);
 *   PK_SPLIT_POS_ASCENDING (8): without RANDOM_LO, key_lo = pos (the first row first).
 * Order values are finite fp64 compared as numbers (-0.0 = +0.0); pos >= 0.
 * pk_segment_select: flags[q] = 1 for the min(k, len) entries of every segment [seg_ptr[s], seg_ptr[s + 1]) with the
 * smallest (key_hi, key_lo) (lexicographic, unsigned), every other of the n flags 0.  Keys must be distinct inside a
 * segment; the result is then unique and reproducible bit for bit.  1 <= k < 2^31, n < 2^32 - 1, empty segments allowed,
 * a segment may be as long as n; seg_ptr ascends within [0, n] (a segment that does not is skipped).
 * work >= pk_segment_select_work_bytes(n_seg, n). */
#define PK_SPLIT_ASCENDING 1
#define PK_SPLIT_RANDOM_LO 2
#define PK_SPLIT_NO_ORDER 4
#define PK_SPLIT_POS_ASCENDING 8
int pk_split_keys(void *stream, int64_t n, const double *order_vals_dev, const int64_t *pos_dev, int32_t mode, uint64_t seed,
                  uint64_t *key_hi_dev, uint64_t *key_lo_dev);
int64_t pk_segment_select_work_bytes(int64_t n_seg, int64_t n);
int pk_segment_select(void *stream, int64_t n_seg, int64_t n, const int64_t *seg_ptr_dev, const uint64_t *key_hi_dev,
                      const uint64_t *key_lo_dev, int64_t k, uint8_t *flags_dev, void *work_dev);
/* vals_out[p] = (row_scale[row of p] * vals[p]) * col_scale[indices[p]] (fp64): the diagonal rescaling A' = D_r A D_c of
 * ScaledMatrixMixin (models.py:864-895, preprocessing/matrices.py:71-93) applied to the device CSR. */
int pk_csr_scale_f64(void *stream, int64_t n_rows, const int64_t *indptr_dev, const int32_t *indices_dev, const void *vals_dev,
                     int val_kind, const double *row_scale_dev, const double *col_scale_dev, double *vals_out_dev);
/* Wave-task plan of a CSR (one 64-lane wave per task, rows longer than `split` cut into near-equal tasks whose
 * partial results are added in slot order): phase 1 leaves counts_dev[0..2] = (tasks, long rows, slots), phase 2
 * fills the arrays sized from them.  row_first_task / row_long_index (int64[n_rows + 1], optional) = first task of
 * a row / number of long rows before it, so that a row range can run as its own launch. */
int64_t pk_row_plan_work_bytes(int64_t n_rows);
int pk_row_plan_count(void *stream, int64_t n_rows, const int64_t *indptr_dev, int32_t split, int64_t *counts_dev,
                      void *work_dev);
int pk_row_plan_fill(void *stream, int64_t n_rows, const int64_t *indptr_dev, const void *work_dev,
                     int32_t *task_row_dev, int64_t *task_begin_dev, int64_t *task_end_dev, int32_t *task_slot_dev,
                     int32_t *long_row_dev, int32_t *long_slot_begin_dev, int32_t *long_slot_end_dev,
                     int64_t *row_first_task_dev, int64_t *row_long_index_dev);

/* ------------------------------------------------------------------------------------------
 * K2.  Dense tall-skinny fp64 pieces of the block eigensolver / HOOI.
 * Replace: ARPACK's Fortran re-orthogonalisation + LAPACK QR/SVD inside `svds`
 * (models.py:844; lib/tensor.py:71,75,79) and numpy `qr` (tensor.py:61,63).
 * ------------------------------------------------------------------------------------------ */
/* G[la x lb] = A^T B, A: n x la, B: n x lb.  work >= pk_gram_work_bytes(n, la, lb). */
int64_t pk_gram_work_bytes(int64_t n, int32_t la, int32_t lb);
int pk_gram_f64(void *stream, int64_t n, int32_t la, int32_t lb, const double *A_dev, int64_t lda,
                const double *B_dev, int64_t ldb, double *G_dev, int64_t ldg, void *work_dev);
/* out[n x lout] = X[n x lin] * C[lin x lout]   (out must not alias X) */
int pk_tsmm_f64(void *stream, int64_t n, int32_t lin, int32_t lout, const double *X_dev, int64_t ldx,
                const double *C_dev, int64_t ldc, double *out_dev, int64_t ldo);
/* out[n x lout] = Z[n x lout] - X[n x lin] * C[lin x lout]  (out may alias Z, not X): the projection X - V (V^T X) of the
 * solvers in one pass */
int pk_tsmm_sub_f64(void *stream, int64_t n, int32_t lin, int32_t lout, const double *X_dev, int64_t ldx,
                    const double *C_dev, int64_t ldc, const double *Z_dev, int64_t ldz, double *out_dev, int64_t ldo);
/* out = alpha X C + beta Z1 + gamma Z2 in one pass (Z1 / Z2 may be NULL): one step of the Chebyshev recurrence on a small
 * dense operator — the projected problems of the block Lanczos build (ARPACK solves the same projected problem inside
 * svds, models.py:844) — in ONE launch instead of a Gram product, its reduction and the recurrence. */
int pk_tsmm_axpby_f64(void *stream, int64_t n, int32_t lin, int32_t lout, const double *X_dev, int64_t ldx,
                      const double *C_dev, int64_t ldc, double alpha, double beta, const double *Z1_dev, int64_t ldz1,
                      double gamma, const double *Z2_dev, int64_t ldz2, double *out_dev, int64_t ldo);
/* The bookkeeping of an orthonormalisation pass on the device, one launch: flags[0] += sum |info[i]| (Cholesky verdicts),
 * flags[1] = max(flags[1], max |G - I|) (NaN / inf count as 1), info[0..n_info) zeroed for the next block. */
int pk_orth_check_f64(void *stream, int32_t l, const double *G_dev, int64_t ldg, int32_t *info_dev, int32_t n_info,
                      double *flags_dev);
/* Symmetric positive semi-definite eigen-decomposition by one-sided Jacobi, single workgroup.
 * S (n x n, destroyed) -> evals[n] descending, evecs (n x n, ROW i = i-th eigenvector).
 * info_dev[0] = sweeps used, info_dev[1] = 1 if converged.  n <= 1024. */
int pk_eigh_psd_f64(void *stream, int32_t n, double *S_dev, int64_t lds_, double *evecs_dev, int64_t ldv,
                    double *evals_dev, int32_t max_sweeps, double tol, int32_t *info_dev);
/* Same solve; beyond 136 columns (block Jacobi) every round is a launch of its own instead of ONE cooperative launch with
 * grid barriers: the form to re-run when pk_eigh_psd_f64 reports info_dev[1] = 0 there (a barrier that did not complete). */
int pk_eigh_psd_rounds_f64(void *stream, int32_t n, double *S_dev, int64_t lds_, double *evecs_dev, int64_t ldv,
                           double *evals_dev, int32_t max_sweeps, double tol, int32_t *info_dev);
/* The r LEADING eigenpairs of a symmetric PSD matrix in one launch (Householder tridiagonalisation, Sturm-count
 * multisection, inverse iteration, back-transformation; csrc/eigh_top.hip) — what the HOOI unfoldings need of their Gram
 * matrices (the k = r of `svds(unfolding, k=r)`, lib/tensor.py:70-80).  S (n x n) is read only; evals[0..r) descending,
 * ROW j of evecs = j-th eigenvector.  The kernel checks its result against S: info_dev[0] = 1 when it passed, 0 when
 * nothing usable was written (degenerate or pathological input) — the caller then uses pk_eigh_psd_f64.
 * pk_eigh_top_supported: 8 <= n <= 176, 1 <= r <= min(32, n).  work: pk_eigh_top_work_bytes(n) bytes. */
int pk_eigh_top_supported(int32_t n, int32_t r);
int64_t pk_eigh_top_work_bytes(int32_t n);
int pk_eigh_top_f64(void *stream, int32_t n, const double *S_dev, int64_t lds_, int32_t r, double *evecs_dev, int64_t ldv,
                    double *evals_dev, void *work_dev, int32_t *info_dev);
/* Cholesky of a small SPD Gram matrix and the inverse of its factor: G + shift_rel*trace(G)*I = R^T R, Rinv = R^-1 (upper
 * triangular), so that X <- X Rinv is orthonormal (CholeskyQR; replaces LAPACK's QR inside svds / numpy.qr,
 * models.py:844, tensor.py:61).  info_dev[0] = 0 or (column + 1) of the first non-positive pivot.
 * work: pk_chol_work_bytes(n) bytes (0 for n <= 136). */
int64_t pk_chol_work_bytes(int32_t n);
int pk_chol_rinv_f64(void *stream, int32_t n, const double *G_dev, int64_t ldg, double shift_rel, double *Rinv_dev,
                     int64_t ldr, void *work_dev, int32_t *info_dev);
/* The same on the column-scaled matrix D G D, D = diag(G)^-1/2 (unit diagonal): Rinv = D R'^-1, so X Rinv is orthonormal all the
 * same, but the factorisation sees the conditioning of the scaled block (columns of very different norm that are otherwise
 * nearly orthogonal — filtered Ritz vectors — need one pass where the unscaled form needs two).  shift_rel is relative to
 * trace(D G D) = n.  A non-positive diagonal entry of G is reported like a non-positive pivot. */
int pk_chol_rinv_scaled_f64(void *stream, int32_t n, const double *G_dev, int64_t ldg, double shift_rel, double *Rinv_dev,
                     int64_t ldr, void *work_dev, int32_t *info_dev);
/* out = alpha*Z + beta*Y + gamma*X over n_elems (Chebyshev three-term recurrence); Y/X may be NULL */
int pk_axpbypcz_f64(void *stream, int64_t n_elems, double alpha, const double *Z_dev, double beta,
                    const double *Y_dev, double gamma, const double *X_dev, double *out_dev);
/* partial[b, j] = sum over row block b of (Z[i,j] - theta[j]*X[i,j])^2 ; nblocks = pk_resid_blocks(n) */
int32_t pk_resid_blocks(int64_t n);
int pk_resid_colnorm2_f64(void *stream, int64_t n, int32_t l, const double *Z_dev, int64_t ldz,
                          const double *X_dev, int64_t ldx, const double *theta_dev, double *partial_dev);
/* small general C = op(A) op(B) (any shape, one thread per output; for l x l glue only) */
int pk_dgemm_small_f64(void *stream, int transA, int transB, int32_t M, int32_t N, int32_t K,
                       const double *A_dev, int64_t lda, const double *B_dev, int64_t ldb,
                       double *C_dev, int64_t ldc);
/* X[i, j] *= s[j] */
int pk_scale_cols_f64(void *stream, int64_t n, int32_t l, double *X_dev, int64_t ldx, const double *s_dev);

/* ------------------------------------------------------------------------------------------
 * K3.  Fused scoring: scores = E V^T (fp32 MFMA) + seen-item masking + per-user top-k,
 * then exact fp64 re-scoring of the surviving candidates.  No dense score matrix ever exists.
 *
 * Replaces, per user chunk: `(test_matrix.dot(v)).dot(v.T)` (models.py:860),
 * `downvote_seen_items` (models.py:494-519) and `get_topk_elements`/`topsort`
 * (models.py:488-491, 561-563), i.e. the body of `_slice_recommender` (models.py:359-371).
 * ------------------------------------------------------------------------------------------ */
/* number of float elements of the MFMA-fragment-packed image of an [n x K] factor matrix */
int64_t pk_pack_elems(int64_t n, int32_t K);
int32_t pk_pack_kq(int32_t K); /* K padded to a multiple of 8, divided by 8 */
/* src f64 [n x K] (ld) -> packed f32 fragments (32 rows per tile, zero padded) */
int pk_pack_frag_f32(void *stream, int64_t n, int32_t K, const double *src_dev, int64_t ld, float *dst_dev);
/* candidate capacity (power of two in {16,32,64}) used for a given topk; 0 if topk unsupported */
int32_t pk_candidate_capacity(int32_t topk);
/* Streams all item tiles against 32-user groups; keeps the KC best (fp32 score, item) pairs of
 * each user among items NOT in the user's seen list (seen_ptr == NULL: no filtering).
 * cand_* are [splits x n_users_pad x KC] with n_users_pad = 32*ceil(n_users/32); unused slots have
 * idx -1.  `splits` = S > 1 deals the 32-item tiles of the catalogue round-robin to S sweeps per user group
 * (split h takes tiles h, h+S, ...), each with its own wave and threshold (more, smaller work items when
 * there are few users; interleaved so that every sweep meets the high-norm head first and the exact pruning
 * keeps working); the per-split lists are merged by pk_rescore_f64.
 * seen lists must be sorted ascending per user (CSR canonical form).
 * The item range is swept in chunks of `tiles_per_chunk` 32-item tiles, one launch per chunk, so the
 * packed item factors of a chunk stay resident in the 4 MiB per-XCD L2 while every workgroup streams
 * them; the per-user selection state is parked in `state_dev` between launches.  0 = auto: L2-sized chunks for a
 * full sweep, ONE launch for a pruned one (its groups are spread over the head of the catalogue whatever the launches
 * do, and every boundary parks and restores the lists; pk_score_chunk_launches tells the count).
 * Threshold bootstrap: a sweep that starts cold first scores its first 16 tiles WITHOUT selecting — every lane keeps the
 * KC / 2 largest group maxima in a sorted register list — and starts from the smallest of a user's KC values, a lower
 * bound of its final KC-th best score: a quarter of the pushes and flush sorts of a cold start (pk_set_option
 * "score_boot_tiles" overrides; 0 = off).  Should such a sweep end without a full list, the last slot of the list holds idx -2 and
 * pk_rescore_f64 sends the user to the exact path. */
int64_t pk_score_state_bytes(int64_t n_users, int32_t splits);
/* recommended number of item splits for this many users (1 when the users alone fill the chip) */
int32_t pk_score_splits(int64_t n_users, int32_t KC);
/* Seen-item lists (the rows of the test CSR: everything downvote_seen_items masks, models.py:494-519)
 * folded into ONE 64-bit record per 32-item tile a user has seen items in: (tile << 32) | item mask.
 * tiles_dev has the capacity of seen_idx_dev and is addressed by the same seen_ptr_dev; the records
 * of user u are tiles_dev[seen_ptr[u] .. seen_ptr[u] + ntiles_dev[u]).  rows_sorted = 1: every row ascending
 * by item (canonical CSR); 0: any order within a row (columns only renamed, e.g. to a serving index). */
int pk_seen_tiles_build(void *stream, int64_t n_users, const int64_t *seen_ptr_dev, const int32_t *seen_idx_dev,
                        int32_t rows_sorted /* 0: rows in arbitrary item order, sorted in LDS */,
                        int64_t max_row_len /* only read when rows_sorted == 0: <= pk_seen_tiles_max_unsorted_row() */,
                        uint64_t *tiles_dev, int32_t *ntiles_dev);
int32_t pk_seen_tiles_max_unsorted_row(void);
/* The candidate sweep as ONE launch sequence: pk_score_candidates_f32 covers the single sweep with or without item splits,
 * with or without the settle rule at a group's exit.  Every choice is an argument, NULL or 0 = not used, and every rule below
 * is checked before anything is launched.
 *
 * The users' side is given in exactly one of two forms:
 *   packed    Ep_dev: the MFMA fragments of E (pk_pack_frag_f32 / pk_pack_frag_bound_f32), with user_bound_dev [n_users] or
 *             NULL — user_bound_dev and tile_bound_dev go together (both: pruned sweep; neither: full sweep).  E_dev, extra_dev,
 *             user_bound_out_dev and settle must be NULL: nothing would read or write them.
 *   rows      E_dev: the fp64 ROWS of E = test_matrix.dot(v) (models.py:860) as the fold-in leaves them: every wave builds
 *             its 32 users' MFMA fragments and pruning bounds in its prologue — the arithmetic of pk_pack_frag_bound_f32, bit
 *             for bit: bound_u = ||E[u, :K]|| (1 + 1e-6) + extra_scale * extra[u * extra_ld] — so a pass needs neither the
 *             packing launch nor a packed copy of E.  E_dev 16-byte aligned, lde even and >= K; extra_dev: the error weight
 *             column of an approximate fold-in (extra_ld >= 1), or NULL; tile_bound_dev == NULL: full sweep (no pruning).
 *             Ep_dev and user_bound_dev must be NULL.
 *             user_bound_out_dev (float [n_users], or NULL): the users' side of the pruning bound is left there: bound_u
 *             above, an upper bound of ||E_u|| — four bytes per user, stored by the sweep's prologue, for pk_rescore_f64.
 * pk_sweep_takes_rows(): 1 when the sweeps of this library take the rows form; a probe build of csrc/experiments/ returns 0,
 * refuses E_dev, and its callers pack fragments first.
 *
 * settle (or NULL; rows form only): the settle rule of the first re-scoring (pk_rescore_f64) applied where a group of 32
 * users LEAVES the sweep, to the final sorted lists the wave still holds: single sweep (splits = 1, one list per user), KC = 16
 * or 32, 1 <= topk <= KC, vmax >= 0, n_users within int32, pruning bound (tile_bound_dev) and error weights (extra_dev)
 * required.  A user whose order the sweep's own scores decide is SETTLED: its topk ids go to row u of out_idx (row out_perm[u]
 * when given), flags[u] = 8, and its row of cand_score / cand_idx is NOT written (stale).  Every other user keeps its candidate
 * row and is appended to open_list (int32 [n_users], arbitrary order) behind the device counter open_count, which the caller
 * zeroes in front of the sweep (pk_zero_i32, or pk_fold_q20_zero).  The first re-scoring then takes open_list / open_count as
 * its row list; the settled set, the flags and the lists are those of the tier in the re-scoring kernel.
 * pk_sweep_settles(KC): 1 when a host layer should take this route — KC fits and the options "sweep_settle" and
 * "rescore_settle" (pk_set_option, default 1) are on; the entry itself settles whenever it is given the block. */
typedef struct PkSweepSettle {
    int32_t topk;
    double vmax;                 /* v_row_norm_max of the re-scoring entries */
    const float *item_norm;      /* float [n_items] upper bounds of the item rows' norms, or NULL */
    int64_t *out_idx;            /* [n_users x topk] */
    const int64_t *out_perm;     /* [n_users] or NULL */
    int32_t *flags;              /* [n_users] */
    int32_t *open_list;          /* [n_users] */
    int32_t *open_count;         /* [1], zero at the start of the sweep */
} PkSweepSettle;
int pk_sweep_takes_rows(void);
int pk_sweep_settles(int32_t KC);
int pk_score_candidates_f32(void *stream, int64_t n_users, int64_t n_items, int32_t K, const float *Vp_dev,
                            const float *Ep_dev, const float *user_bound_dev /* packed */,
                            const double *E_dev, int64_t lde, const double *extra_dev, int64_t extra_ld, double extra_scale,
                            float *user_bound_out_dev /* rows */,
                            const int64_t *seen_ptr_dev, const uint64_t *seen_tiles_dev,
                            const int32_t *seen_ntiles_dev /* all three NULL: nothing is masked */,
                            int32_t KC, int32_t splits /* splits*KC <= 64 */,
                            float *cand_score_dev, int32_t *cand_idx_dev /* [splits][n_users_pad][KC] */,
                            void *state_dev /* pk_score_state_bytes(n_users, splits) */,
                            int32_t tiles_per_chunk /* 0 = auto */,
                            const float *tile_bound_dev /* [ceil(n_items/32)] or NULL */,
                            const uint32_t *seen_dense_dev, const int32_t *seen_skip_dev,
                            int32_t dense_tiles /* pk_seen_dense_build output, or NULL, NULL, 0: the stream serves every tile */,
                            const PkSweepSettle *settle /* or NULL */);
/* The pruned sweep in TWO PHASES (replaces the same reference lines: the chunk loop body of models.py:359-371, with
 * downvote_seen_items :494-519 and topsort :488-491 fused in).  A launch of the single sweep lasts as long as its slowest
 * wave — the groups of the heaviest users stay ~270 tiles in the sweep, everybody else 70-130 — so the catalogue is
 * cut: tiles [0, head_tiles) are swept once per group (lists + thresholds in slot 0), the remaining tiles are dealt
 * round-robin to `splits` sweeps per group that all START from the head's threshold (a score below it cannot be among
 * the KC best, whatever a split's own list holds), and the splits + 1 lists of a user are merged into ONE list of KC
 * candidates with exact comparisons: the dependent chain of a group is head + tail / splits tiles at the same number
 * of tile-waves.  The merged list is what pk_rescore_f64 takes with splits = 1.
 *   work_*   [(splits + 1)][n_users_pad][KC] raw lists;  cand_*  [n_users_pad][KC] merged;
 *   state    pk_score_state_bytes(n_users, splits + 1): records of slot 0 = the head, slots 1.. = the splits (first int64
 *            of a record: the tile at which the group left that sweep; a head exit below head_tiles means the group was
 *            pruned inside the head and its splits did not run).
 * The users' side: packed or rows, with the rules of pk_score_candidates_f32 (user_bound_out_dev as there); the pruning
 * bounds are required — user_bound_dev and tile_bound_dev with Ep_dev, tile_bound_dev with E_dev — and 1 <= head_tiles <
 * ceil(n_items / 32).  There is no settle block: the rule needs the one final list of a single sweep.
 * pk_score_two_phase_plan: the default (head_tiles, splits) for a user set and a catalogue; head_tiles = 0: use the single
 * sweep (user sets that fill the chip's wave slots on their own: there the sweep is bound by the work of the head tiles,
 * not by its longest chain, and the scheme was measured slower). */
int pk_score_two_phase_plan(int64_t n_users, int64_t n_items, int32_t KC, int32_t *head_tiles, int32_t *splits);
int pk_score_two_phase_f32(void *stream, int64_t n_users, int64_t n_items, int32_t K, const float *Vp_dev,
                           const float *Ep_dev, const float *user_bound_dev /* packed */,
                           const double *E_dev, int64_t lde, const double *extra_dev, int64_t extra_ld, double extra_scale,
                           float *user_bound_out_dev /* rows */,
                           const int64_t *seen_ptr_dev, const uint64_t *seen_tiles_dev, const int32_t *seen_ntiles_dev,
                           int32_t KC, int32_t head_tiles, int32_t splits /* (splits + 1) * KC <= 256 */,
                           float *work_score_dev, int32_t *work_idx_dev, float *cand_score_dev, int32_t *cand_idx_dev,
                           void *state_dev, int32_t tiles_per_chunk /* 0 = auto */,
                           const float *tile_bound_dev /* required */,
                           const uint32_t *seen_dense_dev, const int32_t *seen_skip_dev, int32_t dense_tiles);
/* Dense seen masks for the first dense_tiles tiles of the catalogue — where the sweep spends its time, and where a user
 * has a record in nearly every tile: dense_dev[(u / 32 * dense_tiles + tile) * 32 + u % 32] = the user's 32-bit mask in
 * that tile (one coalesced 128-byte load per tile and wave instead of a cursor walk with a scattered 8-byte load per
 * lane), skip_dev[u] = the user's stream records below dense_tiles.  dense_dev: pk_seen_dense_bytes(n_users, dense_tiles). */
int64_t pk_seen_dense_bytes(int64_t n_users, int32_t dense_tiles);
int pk_seen_dense_build(void *stream, int64_t n_users, const int64_t *seen_ptr_dev, const uint64_t *seen_tiles_dev,
                        const int32_t *seen_ntiles_dev, int32_t dense_tiles, uint32_t *dense_dev, int32_t *skip_dev);
/* launches pk_score_candidates_f32 issues for these arguments (fixed item chunks; doubling chunks when the
 * pruning bounds are passed) */
int32_t pk_score_chunk_launches(int64_t n_items, int32_t K, int32_t splits, int32_t tiles_per_chunk, int32_t pruned);
/* Exact pruning bounds for pk_score_candidates_f32 (Cauchy-Schwarz: |E_u . V_i| <= ||E_u|| ||V_i||).
 * The reference scores every item for every user (models.py:860); the sweep may instead stop, per
 * group of 32 users, at the first tile from which  ||E_u|| * max_{i >= tile} ||V_i||  can no longer
 * beat the user's current KC-th best score.  Both bounds are rounded UP, so the candidate lists — and
 * the certification done by pk_rescore_f64 — are exactly those of the full sweep.
 *   pk_row_norm_bound_f32:  out[r] >= ||src[r,:]||_2                       (user_bound from E)
 *   pk_tile_norm_bound_f32: out[t] >= max_{i >= 32 t} ||V[i,:]||_2         (tile_bound; work: float[n_items])
 * The bound falls fastest when the internal item order is by descending popularity or norm. */
/* After the pass, the state buffer holds, for split h and user group g (32 users), 64 records of 16
 * bytes starting at byte ((h * n_groups + g) * 64) * 16; the first int64 of each record is the tile at
 * which that group left the sweep (absolute tile index; >= n_tiles - S + 1 when it was never pruned): split h
 * scored ceil((that - h) / S) tiles, for the roofline accounting of bench.py. */
int pk_row_norm_bound_f32(void *stream, int64_t n, int32_t K, const double *src_dev, int64_t ld, float *out_dev);
/* The fp32 image of the item factors the approximate fold-in gathers from: out [n x ld32] (ld32 > K) = fl32(V) in columns
 * 0..K-1, bound_dev[r] (pk_row_norm_bound_f32) in column K, zeros beyond.  stat_dev[2] (uint32): [0] = the bits of the largest
 * bound, [1] != 0 when an entry of V or a bound is not finite — the range check of the image in the same launch. */
int pk_v32_image_f32(void *stream, int64_t n, int32_t K, int32_t ld32, const double *V_dev, int64_t ldv, const float *bound_dev,
                     float *out_dev, uint32_t *stat_dev);
/* pk_pack_frag_f32 and the row bound in one pass over the block (the user side of a scoring pass):
 * bound[r] >= ||src[r,:]||_2 + extra_scale * extra[r * extra_ld]   (extra_dev may be NULL). */
int pk_pack_frag_bound_f32(void *stream, int64_t n, int32_t K, const double *src_dev, int64_t ld, float *dst_dev,
                           float *bound_dev, const double *extra_dev, int64_t extra_ld, double extra_scale);
int pk_tile_norm_bound_f32(void *stream, int64_t n_items, int32_t K, const double *V_dev, int64_t ld,
                           float *work_dev, float *out_dev);
/* Exact fp64 re-scoring + final ordering (score desc, item asc) of the candidate lists: ONE entry.  Every choice is an
 * argument (NULL = not used) and nothing is kept between two calls.  Writes topk item ids (int64) and
 * optionally their fp64 scores.  flags[u] != 0 marks users whose result is NOT guaranteed exact by
 * the fp32 candidate pass (bit0: candidate margin below the fp32 error bound; bit1: fewer than
 * topk unseen items) — those are re-run through pk_score_exact_rows_f64 / pk_score_exact_list_f64.
 * v_row_norm_max = max_i ||V[i,:]||_2 (<= 1 for orthonormal factors) enters the fp32 error bound.
 * The plain call over everybody with exact E rows: n_rows = n_users, e_exact = 0, flagged_offset = 0, ldv32 = e_err_ld = 0 and
 * every optional pointer (rows, n_rows, V32, e_err, out_score, flagged_list / _count, item_norm, out_perm, user_norm) NULL.
 *
 * rows_dev: the r-th row processed is user rows_dev[r] (NULL: user r, n_rows = n_users) — used to re-do a
 * list of users; n_rows_dev (or NULL): the list length is then min(*n_rows_dev, n_rows), read on the device.
 * e_err_dev (or NULL): per-user bound w_u (that of user u at e_err_dev[u * e_err_ld]) such that the given E rows satisfy
 * ||E'_u - E_u|| <= 2^-24 w_u (the approximate fold-in against fl32(V): w_u = sum_j |a_uj| ||V_j||).  Scores are
 * then within delta_u = 2^-24 w_u max||V_i|| of the exact ones, and flags bit2 (value 4) marks the users whose
 * order is NOT certified at that accuracy (two consecutive scores of the top-k, or the k-th and the best
 * excluded item, closer than 2 delta_u): the caller recomputes their E rows exactly and calls again with
 * e_exact = 1 (these E rows are exact, the candidates came from a sweep over approximate ones; the same e_err_dev: the
 * non-candidates are still only known through the approximate sweep).
 * V32_dev (or NULL): fl32 image of the item factors [n_items x ldv32]; used INSTEAD of V_dev in a first call over
 * approximate E rows (e_err_dev given, e_exact = 0) — half the cache lines per gathered row; its rounding,
 * 2^-24 ||E'_u|| max||V_i||, is added to delta_u.  Ignored when the E rows are exact.
 * flagged_list_dev / flagged_count_dev (both or neither): the users the call flags are appended to a device-side list while
 * it runs: flagged_list_dev[old *count ...] = flagged_offset + user for every user whose flag is not 0 (order arbitrary),
 * *flagged_count_dev advanced by an atomic — what pk_flag_compact(mask = all) makes of the flags afterwards, without its
 * two launches.  The counter is NOT zeroed here (several calls may append to one list: user batches): pk_zero_i32
 * (n <= 2^20 counters, a kernel) first.
 * item_norm_dev (or NULL): the items' own norm bounds, item_norm_dev[i] >= ||V_i|| (fp32, e.g. pk_row_norm_bound_f32) — the
 * order of two neighbouring entries is then certified against cu (||V_i|| + ||V_i'||) instead of 2 cu max ||V||
 * (cu = 2^-24 (e_err[u] + ||E'_u||)): fewer users to re-fold for the same proof.
 * out_perm_dev (int64 [n_users], or NULL): the out_idx row of user u is written to row out_perm_dev[u]; the rows
 * of out_score and flags stay where they are.  A pass that sweeps its users in another order than the caller's then needs
 * no pk_scatter_rows_i64 behind it.
 * user_norm_dev (float [n_users], or NULL): the SETTLE TIER.  It holds N_u >= ||E'_u||, the users'
 * side of the sweep's pruning bound (pk_pack_frag_bound_f32's bound_dev, or what a sweep left in user_bound_out_dev).  Active
 * only on the first call over an approximate E — V32_dev and e_err_dev given, e_exact = 0, rows_dev = NULL.  The sweep's
 * fp32 score of an item is within d_i = (B N_u + 2^-24 e_err[u]) n_i of its exact score, B = 3 * 2^-16 + (4 K + 10) * 2^-23,
 * n_i = item_norm[i] or v_row_norm_max.  A user whose candidates, sorted by their sweep scores, keep more than d + d'
 * between neighbours down to the (topk+1)-th, between the topk-th and every later entry, and between the topk-th and the
 * bound on the items the sweep left out (tau_cert: d_topk + d at n = v_row_norm_max) is SETTLED: its ids are written in that
 * order — the exact one — without gathering an item row or reading its row of E; flags[u] = 8 (above the mask 7 of the
 * lists: such a user is on no list), its out_score row is not written.  Ties, unbounded lists and users with fewer than
 * topk unseen items never settle and take the path of a call without user_norm_dev, bit for bit.
 * pk_set_option("rescore_settle", 0) switches the tier off in every call. */
int pk_rescore_f64(void *stream, int64_t n_rows, const int32_t *rows_dev, const int32_t *n_rows_dev,
                   int64_t n_users, int64_t n_items,
                   int32_t K, const double *V_dev, int64_t ldv,
                   const float *V32_dev, int64_t ldv32,
                   const double *E_dev, int64_t lde,
                   const double *e_err_dev, int64_t e_err_ld, int32_t e_exact,
                   const int64_t *seen_ptr_dev, int32_t KC, int32_t splits,
                   const float *cand_score_dev, const int32_t *cand_idx_dev, int32_t topk,
                   double v_row_norm_max,
                   int64_t *out_idx_dev, double *out_score_dev, int32_t *flags_dev,
                   int32_t *flagged_list_dev, int32_t *flagged_count_dev, int32_t flagged_offset,
                   const float *item_norm_dev, const int64_t *out_perm_dev, const float *user_norm_dev);
int pk_zero_i32(void *stream, int32_t *p_dev, int32_t n);
/* The re-do of flagged users without a host round trip: pk_flag_compact lists the users with (flags & mask) != 0
 * (list capacity n, *count_dev = list length), pk_fold_rows_f64 recomputes the listed rows of E = A_test V in fp64
 * straight from the CSR (row = row_offset + list[r]), pk_rescore_f64 re-scores them (rows_dev = the list,
 * n_rows_dev = count_dev).  All three take the list length from device memory. */
int pk_flag_compact(void *stream, int64_t n, const int32_t *flags_dev, int32_t mask, int32_t *list_dev,
                    int32_t *count_dev);
int pk_fold_rows_f64(void *stream, int64_t cap, const int32_t *list_dev, const int32_t *count_dev, int64_t row_offset,
                     const int64_t *indptr_dev, const int32_t *indices_dev, const void *vals_dev, int val_kind,
                     const double *V_dev, int64_t ldv, int32_t K, double *E_dev, int64_t lde);

/* The product restricted to FLAGGED rows: only the tasks of rows r with (row_flags_dev[r] & flag_mask) != 0 run, every
 * other row of `out` is left alone.  The exact re-fold of the users an ids-only pass could not certify at the accuracy
 * of its approximate fold-in (pk_rescore_f64 leaves the flags on the device): same plan, mapping and
 * summation order as pk_spmm_csr_ex with an fp64 dense block, so a re-folded row has the bits of the exact product.
 * Even nc and ldx, X 16-byte aligned (odd ranks: pk_fold_rows_f64). */
int pk_spmm_csr_flagged_f64(void *stream, int64_t n_tasks, const int32_t *task_row_dev, const int64_t *task_begin_dev,
                            const int64_t *task_end_dev, const int32_t *task_slot_dev, int64_t n_long,
                            const int32_t *long_row_dev, const int32_t *long_slot_begin_dev,
                            const int32_t *long_slot_end_dev, const int32_t *indices_dev, const void *vals_dev,
                            int val_kind, const double *X_dev, int64_t ldx, int32_t nc, double *out_dev, int64_t ldo,
                            double *partial_dev, int64_t x_rows, const int32_t *row_flags_dev, int32_t flag_mask);

/* The same product on LISTED rows: list_dev[0 .. min(*count_dev, cap)) names the rows (row = row_offset + list[i]; the list
 * the re-scoring kernel appends the uncertified users to), a wave walks the tasks [row_first_task[row], row_first_task[row + 1])
 * of a listed row — the task arrays are those of the WHOLE plan (pk_row_plan_fill), the long-row arrays those of the row
 * range whose split rows may be listed (their partial sums are added under the same flag predicate as above).  Costs what the
 * listed rows cost: the flag-predicated form launches a wave per task of every row (0.23 ms of early exits on S-1M). */
int pk_spmm_csr_rows_list_f64(void *stream, int64_t cap, const int32_t *list_dev, const int32_t *count_dev, int64_t row_offset,
                              const int64_t *row_first_task_dev, const int32_t *task_row_dev, const int64_t *task_begin_dev,
                              const int64_t *task_end_dev, const int32_t *task_slot_dev, int64_t n_long,
                              const int32_t *long_row_dev, const int32_t *long_slot_begin_dev, const int32_t *long_slot_end_dev,
                              const int32_t *indices_dev, const void *vals_dev, int val_kind, const double *X_dev, int64_t ldx,
                              int32_t nc, double *out_dev, int64_t ldo, double *partial_dev, int64_t x_rows,
                              const int32_t *row_flags_dev, int32_t flag_mask);

/* ------------------------------------------------------------------------------------------
 * K4q.  The approximate fold-in of an ids-only scoring pass against a PACKED image of the item factors
 * (csrc/foldq.hip): E'[u, 0:K] = sum_j a_uj decode(image row j), E'[u, K] = w_u = sum_j a_uj D_j with
 * ||E'_u - E_u|| <= 2^-24 w_u PROVEN (D_j is computed by the encoder from the bits it wrote), columns K+1 .. Kx-1 = 0.
 * Replaces `test_matrix.dot(v)` (models.py:857-860) wherever the pass certifies its lists against that bound
 * (pk_rescore_f64 with e_err = column K; users it cannot certify are re-folded in fp64 by
 * pk_fold_rows_f64).  A rank-K row takes pk_q20_lanes(K) * 16 bytes (128 for K <= 50: ONE cache line per gathered
 * entry where the fp32 image takes two); ranks above 202 have no packed image (pk_q20_lanes returns 0).
 * pk_q20_encode_f64: V [n x K] fp64 row-major -> image (pk_q20_image_bytes, 128-byte aligned), the bracket scale table
 * tab_dev (96 doubles), info_dev (int32: 0 = ok, else the factors are outside the format's range: use the fp32 image);
 * work_dev: 768 bytes.  pk_q20_decode_f64: the rows exactly as the fold-in reads them, [n x (K + 1)], column K = D_j
 * (tests, diagnostics).  pk_fold_q20: the row-task plan of pk_spmm_csr_ex; non-negative values only (w_u is a bound
 * for a_uj >= 0); the partial buffer holds Kx doubles per slot.  Every row a launch touches is written in full: columns
 * 0 .. K, columns K+1 .. Kx-1 as zero, a row without entries as Kx zeros (a row outside the launch's tasks keeps what it held);
 * column K of a row is kappa * (its sum of weight windows), rounded once per task — a split row's is the sum of its
 * tasks' in slot order.  The padded lanes of a task's last chunk (and a task without entries) gather image row 0 with
 * weight 0: row 0 of the image must be allocated, and tab_dev must be finite (0 * tab[b] * window is then 0 whatever the
 * bits of row 0).  Errors (rank above 202, Kx <= K, ldo < Kx, a val_kind other than PK_VAL_F32 / PK_VAL_F64, split rows
 * without a partial buffer, n_items >= 2^24 or an image of 4 GiB) are returned before anything is launched. */
int32_t pk_q20_lanes(int32_t K);
double pk_q20_kappa(int32_t K);
int64_t pk_q20_image_bytes(int64_t n, int32_t K);
int pk_q20_encode_f64(void *stream, int64_t n, int32_t K, const double *V_dev, int64_t ldv, void *img_dev,
                      double *tab_dev, void *work_dev, int32_t *info_dev);
int pk_q20_decode_f64(void *stream, int64_t n, int32_t K, const void *img_dev, const double *tab_dev, double *out_dev,
                      int64_t ldo);
int pk_fold_q20(void *stream, int64_t n_tasks, const int32_t *task_row_dev, const int64_t *task_begin_dev,
                const int64_t *task_end_dev, const int32_t *task_slot_dev, int64_t n_long,
                const int32_t *long_row_dev, const int32_t *long_slot_begin_dev, const int32_t *long_slot_end_dev,
                const int32_t *indices_dev, const void *vals_dev, int val_kind, const void *img_dev,
                const double *tab_dev, int64_t n_items, int32_t K, int32_t Kx, double *out_dev, int64_t ldo,
                double *partial_dev);
/* pk_fold_q20 that also zeroes the int32 counters zero_dev[0 .. zero_n) in its fix-up launch (which then runs even when no
 * row is split): the counters of a scoring pass are first touched behind the sweep, so their reset needs no launch. */
int pk_fold_q20_zero(void *stream, int64_t n_tasks, const int32_t *task_row_dev, const int64_t *task_begin_dev,
                     const int64_t *task_end_dev, const int32_t *task_slot_dev, int64_t n_long,
                     const int32_t *long_row_dev, const int32_t *long_slot_begin_dev, const int32_t *long_slot_end_dev,
                     const int32_t *indices_dev, const void *vals_dev, int val_kind, const void *img_dev,
                     const double *tab_dev, int64_t n_items, int32_t K, int32_t Kx, double *out_dev, int64_t ldo,
                     double *partial_dev, int32_t *zero_dev, int32_t zero_n);
/* pk_fold_q20_zero with `tasks_per_wave` adjacent row tasks sharing one wave: 1 (what the two entries above run), 2 or 4; any
 * other value is refused, and the value is clamped to what the rank's lane class allows (4 up to K = 50, 2 up to K = 101, 1
 * above).  A wave runs as long as the longest of its tasks, so more than one pays only where adjacent tasks are alike in
 * length (a matrix whose rows are in activity order): the caller states that by asking for it.  Every value keeps the
 * contract above (the same certified weight, the same rows written); the bits of columns 0 .. K-1 may differ between
 * values — the order of the fp64 sums — and never between two launches of one value. */
int pk_fold_q20_sliced(void *stream, int64_t n_tasks, const int32_t *task_row_dev, const int64_t *task_begin_dev,
                       const int64_t *task_end_dev, const int32_t *task_slot_dev, int64_t n_long,
                       const int32_t *long_row_dev, const int32_t *long_slot_begin_dev, const int32_t *long_slot_end_dev,
                       const int32_t *indices_dev, const void *vals_dev, int val_kind, const void *img_dev,
                       const double *tab_dev, int64_t n_items, int32_t K, int32_t Kx, double *out_dev, int64_t ldo,
                       double *partial_dev, int32_t *zero_dev, int32_t zero_n, int32_t tasks_per_wave);
/* dst[perm_dev[r], :] = src_dev[r, :] for rows of `width` int64 (perm_dev == NULL: a plain copy): the lists of a pass whose
 * users were grouped by activity go back to the caller's user order.  `dst` is device memory or MAPPED PINNED HOST memory:
 * the host-side [n_users x topk] int64 array of get_recommendations (models.py:400-405) can be written by the kernel
 * itself, without a copy-engine transfer behind the pass. */
int pk_scatter_rows_i64(void *stream, int64_t n_rows, int32_t width, const int64_t *src_dev, const int64_t *perm_dev,
                        int64_t *dst);
/* dst[e] = src_dev[e] >= 0 ? table_dev[src_dev[e]] : -1: internal item positions -> the item ids of the caller's index
 * (the renaming get_recommendations applies to its result, models.py:400-405 return ids of data.index.itemid), on the
 * device; `dst` is device or mapped pinned host memory. */
int pk_map_ids_i64(void *stream, int64_t n, const int64_t *src_dev, const int64_t *table_dev, int64_t n_table, int64_t *dst);
/* Brute-force exact path for a list of users: all n_items fp64 scores, two-class key
 * (unseen above seen, then score; the reference's downvote semantics, models.py:510-519), top-k.
 * Outputs are compact [n_rows x topk] (row r belongs to user rows_dev[r]).
 * work: pk_exact_work_bytes(n_rows, n_items) bytes. */
int64_t pk_exact_work_bytes(int32_t n_rows, int64_t n_items);
int pk_score_exact_rows_f64(void *stream, int32_t n_rows, const int32_t *rows_dev, int64_t n_items,
                            int32_t K, const double *V_dev, int64_t ldv, const double *E_dev, int64_t lde,
                            const int64_t *seen_ptr_dev, const int32_t *seen_idx_dev, int32_t topk,
                            int64_t *out_idx_dev, double *out_score_dev, void *work_dev);
/* The same rows for a DEVICE-side list (pk_flag_compact output): users list_dev[0 .. *count_dev); results go to the rows
 * of those users in the [n_users x topk] outputs.  One launch; n_wg row slots (work >= pk_exact_work_bytes(n_wg, n_items),
 * prepared ONCE with pk_exact_work_init(stream, work, n_wg, n_items): the buffer ends in one int32 ticket per row slot that
 * must be zero at the first use and that every call leaves zero); the list never visits the host, so a scoring pass needs
 * no synchronisation.  A buffer serves one stream at a time.  out_perm_dev (or NULL: rows stay where they are) as in
 * pk_rescore_f64. */
int pk_exact_work_init(void *stream, void *work_dev, int32_t n_rows, int64_t n_items);
int pk_score_exact_list_f64(void *stream, int32_t n_wg, const int32_t *list_dev, const int32_t *count_dev, int64_t n_items,
                            int32_t K, const double *V_dev, int64_t ldv, const double *E_dev, int64_t lde,
                            const int64_t *seen_ptr_dev, const int32_t *seen_idx_dev, int32_t topk, int64_t *out_idx_dev,
                            double *out_score_dev, void *work_dev, const int64_t *out_perm_dev);
/* Evaluation support (models.py:408-485, evaluation.py:24-44 `build_rank_matrix` restricted to the holdout):
 * rank_out[e] = 1-based position of hold_item[e] in row hold_row[e] of the device-resident [n_users x topk]
 * recommendation array, 0 if absent.  Every hit/rank metric is a reduction of this holdout-sized vector. */
int pk_eval_ranks(void *stream, int64_t n_holdout, const int64_t *recs_dev, int32_t topk,
                  const int64_t *hold_row_dev, const int64_t *hold_item_dev, int32_t *rank_out_dev);
/* evaluate() on the device (models.py:408-485; formulas of recommender/evaluation.py:90-253).  One row of 16 doubles
 * per test user: tp, fp, tn, fn (evaluation.py:176-205), precision, recall, fallout, specifity, miss_rate (:208-236),
 * arhr, mrr (:108-118), map (:120-133), ndcg, ndcl (:136-173), valid recommendations, holdout items.
 * recs: [n_users x ld] int64 (negative = padding); the holdout is CSR-like over the SAME user rows (hold_ptr int64
 * [n_users + 1], items in the id space of recs, hold_rel = feedback or NULL (= ones: ignore_feedback), hold_pos =
 * feedback >= switch_positive per entry or NULL (no positive/negative split)).  pk_eval_reduce adds the columns up
 * in a fixed order (work >= pk_eval_reduce_work_bytes); the means are sums / n_users. */
int32_t pk_eval_cols(void);
int pk_eval_user_metrics(void *stream, int64_t n_users, int32_t topk, const int64_t *recs_dev, int64_t ld,
                         const int64_t *hold_ptr_dev, const int64_t *hold_item_dev, const double *hold_rel_dev,
                         const unsigned char *hold_pos_dev, double not_rated_penalty, double switch_positive,
                         int32_t alternative, double *out_dev);
int64_t pk_eval_reduce_work_bytes(int64_t n_users);
int pk_eval_reduce(void *stream, int64_t n_users, const double *table_dev, double *sums_dev, void *work_dev);
/* coverage (evaluation.py:239-242): count_dev[0] = number of distinct ids in [0, n_bins) (+1 when any id is negative: np.unique
 * counts the padding constant too); flags_dev int32[n_bins + 1] scratch */
int pk_unique_count_i64(void *stream, int64_t n, const int64_t *ids_dev, int64_t n_bins, int32_t *flags_dev,
                        int64_t *count_dev);
/* Dense fp64 score rows (kept for `slice_recommendations`/`_user_scores`, models.py:277-291):
 * out[r, :] = E[r, :] V^T for r in [0, n_rows). */
int pk_dense_scores_f64(void *stream, int32_t n_rows, int64_t n_items, int32_t K, const double *V_dev,
                        int64_t ldv, const double *E_dev, int64_t lde, double *out_dev, int64_t ldo);
/* Top-k columns of dense score rows by (score descending, column ascending): get_topk_elements / topsort on an array
 * (models.py:488-491, 561-563; where scores tie the reference's argpartition order is implementation-defined).
 * out_idx_dev int64 [n_rows x topk]. */
int pk_topk_rows_f64(void *stream, int64_t n_rows, int64_t n_cols, const double *scores_dev, int64_t ld, int32_t topk,
                     int64_t *out_idx_dev);

/* ------------------------------------------------------------------------------------------
 * Item-to-item and most-popular baselines (CooccurrenceModel / PopularityModel, models.py:649-666, 699-725; their
 * scores go through downvote_seen_items / get_topk_elements, models.py:494-563, and lib/sparse.py:33-55).
 * Selection everywhere uses ONE total order: class descending (candidate > seen item of the dense branch under
 * filter_seen > not a candidate), score descending, item index ascending; non-candidates come out as -1.
 * ------------------------------------------------------------------------------------------ */
/* Limits and planning (host functions): the largest topk of pk_i2i_topk, the columns of a scoring workgroup, the fp64
 * columns of a build workgroup, the leading dimension of C for n_items (n_items rounded up to a multiple of 8), the
 * users scored per launch pair and the scratch pk_i2i_topk needs. */
int32_t pk_i2i_max_topk(void);
int32_t pk_i2i_window(void);
int32_t pk_i2i_build_window(void);
int64_t pk_i2i_ld(int64_t n_items);
int64_t pk_i2i_chunk_users(int64_t n_users, int64_t n_items, int32_t topk);
int64_t pk_i2i_topk_work_bytes(int64_t n_users, int64_t n_items, int32_t topk);
/* C = A^T A with the diagonal set to 0 (models.py:710-713), dense fp64 [n_items x ldc] (ldc = pk_i2i_ld(n_items); the
 * columns beyond n_items are written as 0).  A: CSR user -> items with sorted columns (indptr, indices, values) and its
 * CSC image item -> users (t_*, pk_csr_transpose), values of kind val_kind in both.  Accumulated in fp64: exact whenever
 * every product and partial sum is representable (integer or half-integer feedback). */
int pk_i2i_build_f64(void *stream, int64_t n_users, int64_t n_items, const int64_t *indptr_dev, const int32_t *indices_dev,
                     const void *values_dev, int val_kind, const int64_t *t_indptr_dev, const int32_t *t_indices_dev,
                     const void *t_values_dev, double *C_dev, int64_t ldc);
/* C32[e] = (float)C64[e] for e < n; *inexact_dev |= 1 (an int32 the caller zeroed) where (double)(float)c != c. */
int pk_i2i_image_f32(void *stream, int64_t n, const double *C64_dev, float *C32_dev, int32_t *inexact_dev);
/* Scores s_u = sum_i t_ui C[i, :] of the n_users rows of the test CSR (t_*: sorted columns, values of kind t_val_kind,
 * zero values kept: they add nothing but count as seen) against C (c_kind = PK_VAL_F32 / PK_VAL_F64, leading dimension
 * ldc = pk_i2i_ld(n_items)), accumulated in fp64, and the top-k of every row:
 *   sparse = 0 (dense branch): every item is a candidate; filter_seen ranks the seen items after all unseen ones;
 *   sparse = 1 (sparse branch): the candidates are the items with a nonzero score, minus the seen ones under filter_seen.
 * out_idx_dev int64 [n_users x topk] (-1 = fewer candidates than topk), out_scores_dev fp64 [n_users x topk] or NULL.
 * 1 <= topk <= pk_i2i_max_topk().  work >= pk_i2i_topk_work_bytes(n_users, n_items, topk). */
int pk_i2i_topk(void *stream, int64_t n_users, int64_t n_items, const int64_t *t_indptr_dev, const int32_t *t_indices_dev,
                const void *t_values_dev, int t_val_kind, const void *C_dev, int c_kind, int64_t ldc, int32_t topk,
                int32_t filter_seen, int32_t sparse, int64_t *out_idx_dev, double *out_scores_dev, void *work_dev);
/* ---- row-wise sparse x sparse product with the top-k fused in (csrc/simagg.hip) -----------------------------------
 * scores[r, :] = sum_p L.values[p] * B[L.indices[p], :] for the rows of a CSR L [n_rows x n_inner] (int64 indptr, int32
 * indices, values of kind l_val_kind, zero values kept) against a canonical CSR B [n_inner x n_cols] (strictly increasing
 * columns per row, fp64 values).  Contract: for every (r, column) the products are added in ascending order of p starting
 * from +0.0, each a separate fp64 multiply and add (no contraction, no atomics), and -0 is stored as +0 — the scores are
 * bit-equal to SciPy's L.dot(B).  n_cols < 2^30. */
/* Scratch of pk_spsp_topk (rows are scored in chunks under the candidate budget of pk_i2i_topk). */
int64_t pk_spsp_topk_work_bytes(int64_t n_rows, int64_t n_cols, int32_t topk);
/* The top-k of every row under the total order of pk_i2i_topk (same classes for sparse = 0 / 1, same pads).  filter_seen
 * marks the row's own stored columns (zero-valued entries included) as seen and is accepted only when n_inner == n_cols.
 * out_idx_dev int64 [n_rows x topk] (-1 = fewer candidates), out_scores_dev fp64 [n_rows x topk] (0 at pads) or NULL.
 * 1 <= topk <= pk_i2i_max_topk().  work >= pk_spsp_topk_work_bytes(n_rows, n_cols, topk). */
int pk_spsp_topk(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                 const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind, const int64_t *b_indptr_dev,
                 const int32_t *b_indices_dev, const double *b_values_dev, int32_t topk, int32_t filter_seen, int32_t sparse,
                 int64_t *out_idx_dev, double *out_scores_dev, void *work_dev);
/* pk_spsp_topk with the seen set handed over: row r of the pattern CSR (seen_indptr_dev int64 [n_rows + 1], seen_indices_dev
 * int32, columns < n_cols ascending per row) holds the seen columns of row r under filter_seen, so n_inner != n_cols is
 * allowed.  Classes, order, pads, score bits and work size are those of pk_spsp_topk; with the pattern of L as the seen set
 * and n_inner == n_cols the two entries return the same bits. */
int pk_spsp_topk_seen(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                      const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind, const int64_t *b_indptr_dev,
                      const int32_t *b_indices_dev, const double *b_values_dev, const int64_t *seen_indptr_dev,
                      const int32_t *seen_indices_dev, int32_t topk, int32_t filter_seen, int32_t sparse, int64_t *out_idx_dev,
                      double *out_scores_dev, void *work_dev);
/* The same sums of rows [row0, row0 + n_rows) of L as a dense fp64 block: out_dev[(r - row0) * ld + c] for c < n_cols
 * (ld >= n_cols; the columns beyond n_cols are not written). */
int pk_spsp_rows_f64(void *stream, int64_t row0, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                     const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind, const int64_t *b_indptr_dev,
                     const int32_t *b_indices_dev, const double *b_values_dev, double *out_dev, int64_t ld);
/* ---- row-wise sparse x sparse product with CSR output and the similarity epilogues (csrc/spgemm.hip) ----------------
 * C = L . B over the operands of pk_spsp_topk, in its summation order, written as a canonical CSR (int64 indptr, int32
 * indices strictly ascending per row, fp64 values).
 *   op        PK_SPGEMM_OP_MUL: acc + v * b, separately rounded (bit-equal to SciPy's product); PK_SPGEMM_OP_MIN: acc + min(v, b).
 *   stored    an entry whose sum is != 0 (-0 is not); with diag = 1 (n_rows == n_cols) entry (r, r) always, as 1.0.
 *   epilogue  of a stored off-diagonal entry with sum s: PK_SPGEMM_EPI_NONE: s; PK_SPGEMM_EPI_JACCARD:
 *             s / ((nf_cols[c] + nf_rows[r]) - s); PK_SPGEMM_EPI_WJACCARD (op = MIN): s / max_sum, max_sum added up as in the
 *             reference's _jaccard_similarity_weighted_tri for the pair (i, j): over the features of j ascending, a matched
 *             one adds max(dat_i, dat_j), an unmatched one dat_j, then the unmatched features of i ascending.
 *             wj_rect = 0: i = min(r, c), j = max(r, c), both rows taken from the CSR f_* (n_rows == n_cols);
 *             wj_rect = 1: j = row r of L, i = row c of f_*.  f_*: the column side's features by item (n_cols rows, sorted
 *             columns, fp64); L's rows must be sorted too.
 * pk_spgemm_count writes C.indptr (n_rows + 1) and keeps the offsets of every (row, window) in work; the caller reads
 * nnz = indptr[n_rows], allocates and calls pk_spgemm_fill with the SAME operands, op, diag and work.  n_cols < 2^30. */
#define PK_SPGEMM_OP_MUL 0
#define PK_SPGEMM_OP_MIN 1
#define PK_SPGEMM_EPI_NONE 0
#define PK_SPGEMM_EPI_JACCARD 1
#define PK_SPGEMM_EPI_WJACCARD 2
int64_t pk_spgemm_work_bytes(int64_t n_rows, int64_t n_cols);
int pk_spgemm_count(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                    const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind, const int64_t *b_indptr_dev,
                    const int32_t *b_indices_dev, const double *b_values_dev, int32_t op, int32_t diag, int64_t *indptr_out_dev,
                    void *work_dev);
int pk_spgemm_fill(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                   const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind, const int64_t *b_indptr_dev,
                   const int32_t *b_indices_dev, const double *b_values_dev, int32_t op, int32_t diag, int32_t epilogue,
                   int32_t wj_rect, const double *nf_rows_dev, const double *nf_cols_dev, const int64_t *f_indptr_dev,
                   const int32_t *f_indices_dev, const double *f_values_dev, const void *work_dev, int64_t nnz,
                   int32_t *out_indices_dev, double *out_values_dev);
/* ---- sampled-negatives evaluation (csrc/sampled.hip; models.py:1095-1183, lib/sparse.py::inner_product_at,
 * lib/sampler.py::mf_random_item_scoring) ------------------------------------------------------------------------------
 * Limits (host functions): the candidates per user the fused launch keeps in LDS, the largest rank, the largest sample. */
int32_t pk_candidates_fused_max(void);
int32_t pk_candidates_max_rank(void);
int32_t pk_sample_max_n(void);
/* Rounds of 64 draws within which every user of pk_sample_unseen is done except with probability below exp(-32), when each
 * has at least min_eligible >= n items to draw from (-1: bad arguments), and the largest limit a launch is accepted with. */
int64_t pk_sample_round_limit(int64_t n_items, int32_t n, int64_t min_eligible);
int32_t pk_sample_max_rounds(void);
/* s[u, c] = sum_f P[u, f] * V[cand[u, c], f] for the C candidates of every user and the top-k of every row.
 * P fp64 [n_users x r], leading dimension ldp; V fp64 [n_items x r]: element (i, f) at V_dev[i * ldv + f * v_col_stride]
 * (row-major: v_col_stride = 1, ldv >= r; column-major: ldv = 1, v_col_stride >= n_items); cand int32 [n_users x C] item
 * ids, NOT range-checked on the device.  Contract: the sum starts from +0.0 and runs over f ascending, each term a
 * separately rounded fp64 multiply and add (no contraction) — bit-equal to the reference's loops for the same P and V.
 * out_idx_dev int64 [n_users x topk]: COLUMN POSITIONS 0..C-1, best first under (score descending, position ascending),
 * the order of pk_topk_rows_f64.  out_scores_dev fp64 [n_users x C] or NULL; required when C > pk_candidates_fused_max()
 * (the selection then runs in pk_topk_rows_f64).  1 <= r <= pk_candidates_max_rank(), 1 <= topk <= C < 2^30. */
int pk_candidates_topk_f64(void *stream, int64_t n_users, int64_t n_items, int32_t r, const double *P_dev, int64_t ldp,
                           const double *V_dev, int64_t ldv, int64_t v_col_stride, const int32_t *cand_dev, int64_t C,
                           int32_t topk, int64_t *out_idx_dev, double *out_scores_dev);
/* n distinct items per user, uniform over the items that are neither in the user's row of the CSR t_* (sorted columns) nor
 * in its row of the CSR h_* (a few entries per row, any order; h_indptr_dev = NULL: no second exclusion), in draw order:
 *   draw t = 0, 1, ...: z = splitmix64 finaliser of (seed_u * 2^32 + t), w = z >> 32, m = w * n_items; the draw is skipped
 *   when (m mod 2^32) < (2^32 mod n_items), else x = m >> 32; x is accepted when it is not excluded and was not accepted
 *   before; the output is the first n accepted x.
 * out_dev int32 [n_users x n]; seeds_dev uint32 [n_users].  min_eligible: a lower bound of n_items - excluded_u over the users,
 * which the caller guarantees to be >= n; it sets the round limit, pk_sample_round_limit(n_items, n, min_eligible) — at most
 * proportional to n_items (1 + ln n) — and a limit above pk_sample_max_rounds() is refused (PK_E_INVALID, no launch).  The
 * caller zeroes *err_dev: a user not done within the limit sets it to 1 and its row is incomplete.  1 <= n <= pk_sample_max_n(). */
int pk_sample_unseen(void *stream, int64_t n_users, int64_t n_items, const int64_t *t_indptr_dev, const int32_t *t_indices_dev,
                     const int64_t *h_indptr_dev, const int32_t *h_indices_dev, int32_t n, int64_t min_eligible,
                     const uint32_t *seeds_dev, int32_t *out_dev, int32_t *err_dev);
/* ---- contextual post-filtering (csrc/context.hip; contextual/models.py:5-32) ----------------------------------------------
 * Limits (host functions): the keys one workgroup sorts at a time, the largest number of contexts. */
int32_t pk_context_window(void);
int32_t pk_context_max(void);
/* The class-lexicographic tier on top of the lists of the scoring pass.  Every user's list is ordered by
 *   class descending, score descending, item ascending,   class = sum_j 2^j [item in the list of the user's value of context j]
 * over the items that are not seen (all items when seen_indptr_dev is NULL); scores are E_u . V_i in fp64 with the summation
 * order of the re-scoring and exact-row kernels (same bits).  The class-0 part comes from base_idx_dev, the lists of the
 * plain pass [n_users x topk] (-1 pads allowed, at the end): out row = the min(topk, emitted) context items of the user,
 * then the base entries that are not among them (in some list of the user and not seen), in their order, up to topk; pads
 * stay at the end.  A seen item is never up-voted: the seen tail of a user with fewer than topk unseen items follows in the
 * base order.
 * V fp64 [n_items x K] rows in serving order (ldv), E fp64 [n_users x K] (lde); seen_*: CSR of the seen items, sorted rows.
 * user_value_dev / value_ptr_dev / value_items_dev: HOST arrays of n_ctx DEVICE pointers; context j: user_value int32
 * [n_users] (-1: no value), value_ptr int64 [n_values + 1], value_items int32 serving positions, ascending and distinct
 * within a value, NOT range-checked on the device.  max_list: the longest list of any value (bounds the rounds of a
 * workgroup).  out_class_dev int32 [n_users x topk] or NULL: the class of every slot, 0 for base entries and pads.
 * order_dev int32 [n_users] or NULL: workgroup b serves row order_dev[b] (a permutation; users of one value next to each other
 * walk the same list).  out_idx_dev must not alias base_idx_dev.
 * 1 <= n_ctx <= pk_context_max(), 1 <= topk <= 1024, 1 <= K <= 1024, n_items < 2^28. */
int pk_context_merge_f64(void *stream, int64_t n_users, int64_t n_items, int32_t K, const double *V_dev, int64_t ldv,
                         const double *E_dev, int64_t lde, const int64_t *seen_indptr_dev, const int32_t *seen_indices_dev,
                         int32_t n_ctx, const int32_t *const *user_value_dev, const int64_t *const *value_ptr_dev,
                         const int32_t *const *value_items_dev, int64_t max_list, const int64_t *base_idx_dev, int32_t topk,
                         int64_t *out_idx_dev, int32_t *out_class_dev, const int32_t *order_dev);
/* The global order of the catalogue for PopularityModel: order_dev[p] = the item at position p by (score descending,
 * item ascending) — one stable device radix sort.  work >= pk_popular_order_work_bytes(n_items). */
int64_t pk_popular_order_work_bytes(int64_t n_items);
int pk_popular_order(void *stream, int64_t n_items, const double *scores_dev, int32_t *order_dev, void *work_dev);
/* The dense branch of PopularityModel (models.py:494-563 on repeated item scores): per test row the first topk items of
 * the global order, with filter_seen the row's unseen items first and its seen items after them in the same order.
 * 1 <= topk <= n_items <= 2^19 (the seen bitmap lives in LDS).  out_idx_dev int64 [n_users x topk]. */
int pk_popular_topk(void *stream, int64_t n_users, int64_t n_items, const int64_t *t_indptr_dev, const int32_t *t_indices_dev,
                    const int32_t *order_dev, int32_t topk, int32_t filter_seen, int64_t *out_idx_dev);

/* ------------------------------------------------------------------------------------------
 * HybridSVD (hybrid/models.py:228-397): a dense Cholesky factor of the item-similarity matrix K = S + beta I and its
 * products.  Every image of K / L is fp64, row-major, with pk_hybrid_ld(n) rows and a leading dimension ld that is a
 * multiple of 64 and at least pk_hybrid_ld(n) (n rounded up to whole 64 x 64 tiles); only the lower triangle is read.
 * ------------------------------------------------------------------------------------------ */
/* Planning (host functions): the rows of an image (n rounded up to a multiple of 64), the largest nc of pk_trmm_f64
 * and the scratch it needs for n rows and nc columns (0: none). */
int64_t pk_hybrid_ld(int64_t n);
int32_t pk_hybrid_max_nc(void);
int64_t pk_trmm_work_bytes(int64_t n, int32_t nc);
/* K = S + beta I in the internal item order: the image is cleared, entry (i, j) of the CSR of S (external ids, int64
 * indptr / indices, no duplicates) is written at (rank[i], rank[j]) when rank[j] <= rank[i], then beta is added on the
 * diagonal. */
int pk_hybrid_densify_f64(void *stream, int64_t n, const int64_t *indptr_dev, const int64_t *indices_dev,
                          const double *data_dev, const int64_t *rank_dev, double beta, double *K_dev, int64_t ld);
/* In-place lower Cholesky K = L L^T of the n x n matrix in A (lower triangle read; on return the strict upper triangle
 * is 0 and the rows / columns of the padding hold the identity).  *info_dev (int32) = -1 on success, else the first
 * column whose pivot is <= 0 or not finite; the work after that column is skipped.  Deterministic. */
int pk_chol_f64(void *stream, int64_t n, double *A_dev, int64_t ld, int32_t *info_dev);
/* Y = L X (trans = 0) or Y = L^T X (trans = 1) for X [n x nc] (1 <= nc <= pk_hybrid_max_nc()), L the factor of
 * pk_chol_f64.  work >= pk_trmm_work_bytes(n, nc); the partial sums of a row are added in a fixed order. */
int pk_trmm_f64(void *stream, int32_t trans, int64_t n, int32_t nc, const double *L_dev, int64_t ld, const double *X_dev,
                int64_t ldx, double *Y_dev, int64_t ldy, void *work_dev);
/* B <- L^-T B in place, B [n x r] with pk_hybrid_ld(n) rows allocated (the rows beyond n are set to 0). */
int pk_trsm_f64(void *stream, int64_t n, int32_t r, const double *L_dev, int64_t ld, double *B_dev, int64_t ldb);

/* ------------------------------------------------------------------------------------------
 * EASE (Steck 2019): B = I - P diag(1 / diag P), P = (X^T X + lambda I)^-1, through the Cholesky image above:
 * pk_i2i_build_f64 writes X^T X (diagonal 0) into the image (ldc = ld), pk_ease_diag_f64 its diagonal, pk_chol_f64
 * factors it, pk_trtri_f64 inverts the factor in place and pk_ease_weights_f64 forms the scoring image of B.
 * Everything is fp64 with a fixed summation order: the results are the same bits from run to run.
 * ------------------------------------------------------------------------------------------ */
/* K[j][j] = sum_u x_uj^2 + lam for j < n_items, from the CSC image of X (t_indptr int64 [n_items + 1], values of
 * val_kind): 16 lanes per item, lane l sums the entries l, l + 16, ... of the column in storage order, the 16 partial sums
 * are added as a fixed tree. */
int pk_ease_diag_f64(void *stream, int64_t n_items, const int64_t *t_indptr_dev, const void *t_values_dev, int val_kind,
                     double lam, double *K_dev, int64_t ld);
/* Scratch of pk_trtri_f64 (host function): the panel product of one block column, one partial block per chunk of 32
 * tiles of a tile row. */
int64_t pk_trtri_work_bytes(int64_t n);
/* In place W = L^-1 of the lower factor pk_chol_f64 left in the image (padding: the identity, so the result is
 * diag(W, I)); the strict upper triangle is not touched.  Block columns are taken last to first; 1 + 2 (n / 64 - 1)
 * launches.  work >= pk_trtri_work_bytes(n). */
int pk_trtri_f64(void *stream, int64_t n, double *L_dev, int64_t ld, void *work_dev);
/* From W = L^-1 (the image of pk_trtri_f64): d_out[j] = P_jj = sum_k W_kj^2 (j < n), and the scoring image
 * B [n x ldb], ldb >= n: B_ij = -P_ij / d_j with P = W^T W summed tile by tile and never stored, B_jj = 0 and the
 * columns [n, ldb) 0. */
int pk_ease_weights_f64(void *stream, int64_t n, const double *W_dev, int64_t ld, double *d_out_dev, double *B_dev,
                        int64_t ldb);

/* ------------------------------------------------------------------------------------------
 * SLIM (Ning & Karypis, ICDM 2011; csrc/slim.hip): the sparse item x item weights W, column by column,
 *     w_j = argmin 1/2 |x_j - X w|^2 + l1 |w|_1 + l2 / 2 |w|^2   subject to w_j[j] = 0 and, with `positive`, w >= 0,
 * by elastic-net coordinate descent over the dense Gram image G = X^T X [n x ldg] WITH its diagonal (pk_i2i_build_f64 +
 * pk_ease_diag_f64 with lam = 0).  The arithmetic is fixed, so that the result does not depend on how it is parallelised
 * (tests/slim_reference.py restates it in NumPy and the device's bits are compared with that).  Everything is fp64 and
 * every product, sum and quotient is rounded on its own (no contraction).  Per target column j, reading row k of the image,
 * G[k][i], wherever a column of G is meant:
 *     w = 0;  r[i] = G[j][i] for all i
 *     for sweep = 1 .. max_sweeps:
 *         dmax = 0; wmax = 0
 *         for k = 0 .. n - 1 in ascending order, k != j:
 *             den = G[k][k] + l2;  if not (den > 0): continue
 *             old = w[k];  rho = r[k] + G[k][k] * old
 *             positive:      t = rho - l1;    new = t > 0 ? t / den : 0
 *             not positive:  t = |rho| - l1;  new = t > 0 ? copysign(t / den, rho) : 0
 *             d = new - old
 *             if d != 0:  r[i] = r[i] - d * G[k][i] for ALL i (k and j included);  w[k] = new
 *             dmax = max(dmax, |d|);  wmax = max(wmax, |new|)
 *         if wmax == 0 or dmax <= tol * wmax: stop
 *     outputs: w, the number of sweeps run
 * A coordinate's update reads one element of r and no reduction, the update of r is element-wise and both maxima are
 * order-free: any implementation that visits the CHANGING coordinates in ascending order produces these bits.  The kernel
 * evaluates 1024 coordinates at once (between two changes r is constant), applies the lowest changing one and continues
 * behind it.
 * ------------------------------------------------------------------------------------------ */
/* Limits and planning (host functions): the largest n of pk_slim_solve_f64 (65 536), the largest n whose residual row r
 * lives in LDS (19 456; beyond it, or with pk_set_option("slim_r_global", 1), r lives in one scratch row per workgroup), the
 * default number of columns of a batch (min(n, 1024)) and the scratch of a solve of nc columns: the diagonal of G
 * (n doubles rounded up to 256 bytes) and, with r in HBM, nc rows of n doubles. */
int64_t pk_slim_max_items(void);
int64_t pk_slim_lds_items(void);
int64_t pk_slim_batch_columns(int64_t n);
int64_t pk_slim_work_bytes(int64_t n, int64_t nc);
/* The target columns [j0, j0 + nc): row c of Wt_block [nc x ldw] (ldw >= n) becomes w_(j0 + c), i.e. row j0 + c of W^T, its
 * columns [n, ldw) exactly 0; sweeps[c] (int32) the sweeps run.  One workgroup per column.  The result of a column does not
 * depend on the batch it is solved in.  work >= pk_slim_work_bytes(n, nc). */
int pk_slim_solve_f64(void *stream, int64_t n, const double *G_dev, int64_t ldg, int64_t j0, int64_t nc, double l1, double l2,
                      double tol, int32_t max_sweeps, int32_t positive, double *Wt_block_dev, int64_t ldw, int32_t *sweeps_dev,
                      void *work_dev);
/* A block [nc x ldw] of rows of W^T as CSR rows: an entry is stored when it is != 0, in ascending index order.
 * pk_slim_csr_count: indptr [nc + 1] (int64, indptr[0] = 0) of the block alone; work >= 8 nc bytes.  pk_slim_csr_fill:
 * indices (int32) and values (fp64) [nnz = indptr[nc]] of the same, unchanged block. */
int pk_slim_csr_count(void *stream, int64_t nc, int64_t n, const double *Wt_block_dev, int64_t ldw, int64_t *indptr_dev,
                      void *work_dev);
int pk_slim_csr_fill(void *stream, int64_t nc, int64_t n, const double *Wt_block_dev, int64_t ldw, const int64_t *indptr_dev,
                     int64_t nnz, int32_t *indices_dev, double *values_dev);

/* ------------------------------------------------------------------------------------------
 * Neighbourhood and random-walk item models (ItemKNN, P3alpha / RP3beta; csrc/knn.hip): one pass over the dense Gram image
 * G [n x ldg] (pk_i2i_build_f64 + pk_ease_diag_f64) that normalises every entry, keeps the K best of every row and writes
 * them as n x K slots — the image is read once, nothing of its size is written.  The arithmetic is fixed
 * (tests/knn_reference.py restates it in NumPy and the device's bits are compared with that): everything is fp64, every
 * product, sum, difference and quotient is rounded on its own (no contraction) and the quotient is the correctly rounded
 * one.  For row i and column j < n, with g = G[i * ldg + j]:
 *     PK_KNN_SCALE:     w = (g * row[i]) * col[j]
 *     PK_KNN_COSINE:    w = g / (row[i] * col[j] + shrink)
 *     PK_KNN_TANIMOTO:  w = g / (((row[i] + col[j]) - g) + shrink)
 *   candidate:  j != i, g != 0, w finite and w != 0
 *   kept:       the min(K, candidates) best by w descending, then j ascending (the total order of pk_topk_rows_f64 and
 *               pk_i2i_topk)
 *   output:     the kept entries in ASCENDING j in the first count[i] slots of row i of idx / val; the other slots are
 *               idx = -1, val = 0
 *   normalize != 0:  s = ((+0.0 + |w_0|) + |w_1|) + ... over the kept entries in ascending j; when s is finite and != 0
 *               every kept w becomes w / s
 * row and col hold n doubles each; every kind reads both.
 * One workgroup per row streams it in windows of pk_i2i_window() columns, sorts a window's keys in LDS and merges its best
 * into the row's running list (the keys, sort and merge of pk_i2i_topk); windows without a candidate that beats the list's
 * last entry are skipped.  No atomics and no cross-workgroup traffic: equal inputs give equal bits.
 * ------------------------------------------------------------------------------------------ */
#define PK_KNN_SCALE 0
#define PK_KNN_COSINE 1
#define PK_KNN_TANIMOTO 2
/* The largest K of pk_knn_prune_f64 (host function): pk_i2i_max_topk() = 1024. */
int32_t pk_knn_max_neighbours(void);
/* count [n] int32; idx [n x K] int32 and val [n x K] fp64, row-major.  1 <= n < 2^30, ldg >= n, 1 <= K <=
 * pk_knn_max_neighbours(), shrink finite and >= 0, no pointer NULL: checked before any device work.  Rows of G are loaded
 * 16 bytes at a time when ldg % 8 == 0 and G and col are 16-byte aligned, one double at a time otherwise: the same bits. */
int pk_knn_prune_f64(void *stream, int64_t n, const double *G_dev, int64_t ldg, int32_t kind, const double *row_dev,
                     const double *col_dev, double shrink, int32_t K, int32_t normalize, int32_t *count_dev, int32_t *idx_dev,
                     double *val_dev);

/* ---- the neighbour pass without an image (csrc/uknn.hip): UserKNN, and ItemKNN / RP3beta with gram = 'sparse' ----------
 * The pruning pass above over a row of L . B formed from the sparse operands of pk_spsp_topk (L: CSR [n_rows x n_inner],
 * int64 indptr, int32 indices, values of kind l_val_kind; B: canonical fp64 CSR [n_inner x n_cols]) instead of a row of
 * an image.  For row r and column c < n_cols:
 *   g           the sum of pk_spsp_topk: the products added in ascending position of the left row from +0.0, each a
 *               separately rounded multiply and add, -0 stored as +0 (an inner index outside [0, n_inner) is skipped)
 *   w           from g, row[r], col[c] and shrink by the three formulas and rounding rules above (no contraction, the
 *               correctly rounded quotient)
 *   candidate   c != exclude[r] (when exclude_dev is given and exclude[r] >= 0), g != 0, w finite and w != 0
 *   kept, output order (ascending c, pads idx -1 / val 0) and normalize: exactly as pk_knn_prune_f64
 * row_dev [n_rows] and col_dev [n_cols] fp64; exclude_dev int32 [n_rows] or NULL; count_dev int32 [n_rows], idx_dev int32
 * [n_rows x K], val_dev fp64 [n_rows x K].  1 <= K <= the largest K of the pruning pass, n_cols < 2^30, shrink finite and
 * >= 0, no other pointer NULL: checked before any device work.  work >= the bytes the work-size function returns.
 * A (row, window) grid accumulates in LDS, forms the keys in place and sorts a touched window; the merge of pk_i2i_topk
 * joins a row's windows and a finishing kernel orders, normalises and writes the slots.  Rows are chunked under the
 * candidate budget of pk_i2i_topk.  No atomics on results, no cross-workgroup ordering: equal inputs give equal bits. */
int64_t pk_spsp_knn_work_bytes(int64_t n_rows, int64_t n_cols, int32_t K);
int pk_spsp_knn_f64(void *stream, int64_t n_rows, int64_t n_inner, int64_t n_cols, const int64_t *l_indptr_dev,
                    const int32_t *l_indices_dev, const void *l_values_dev, int l_val_kind, const int64_t *b_indptr_dev,
                    const int32_t *b_indices_dev, const double *b_values_dev, int32_t kind, const double *row_dev,
                    const double *col_dev, double shrink, const int32_t *exclude_dev, int32_t K, int32_t normalize,
                    int32_t *count_dev, int32_t *idx_dev, double *val_dev, void *work_dev);

/* ------------------------------------------------------------------------------------------
 * Local Collective Embeddings (csrc/lce.hip).  Replace the NumPy element-wise updates and traces of
 * `local_collective_embeddings` (lib/optimize.py:347-379).  The factors are tall row-major fp64 blocks, the H factors
 * transposed ([labels x k], [users x k]), so the three multiplicative updates are one form:
 *     X <- X o (a N) / max(X M + (lamb + c_i) X, 1e-10),    M = ma M1 + mb M2 (k x k; M2 may be NULL)
 *   Hs^T: N = Xs^T W, M = alpha W^T W;  Hu^T: N = Xu^T W, M = gamma W^T W  (optimize.py:350-356)
 *   W:    N = alpha Xs Hs^T + gamma Xu Hu^T + beta A W, M = alpha Hs Hs^T + gamma Hu Hu^T, c = beta d  (optimize.py:359-363)
 * pk_lce_update_f64: ONE launch, M in LDS, k <= pk_lce_fused_max_rank() (128: 128 KiB of the CU's 160 KiB hold M, 16 KiB the
 * staged rows); every row of X and N is read once.  Above that rank: P = X M by pk_tsmm_f64, then pk_lce_update_ew_f64.
 * c_dev: [m] or NULL.  X must not alias N or P. */
int32_t pk_lce_fused_max_rank(void);
int pk_lce_update_f64(void *stream, int64_t m, int32_t k, double *X_dev, int64_t ldx, const double *N_dev, int64_t ldn,
                      const double *M1_dev, int64_t ldm1, double ma, const double *M2_dev, int64_t ldm2, double mb,
                      double a, double lamb, const double *c_dev);
int pk_lce_update_ew_f64(void *stream, int64_t m, int32_t k, double *X_dev, int64_t ldx, const double *N_dev, int64_t ldn,
                         const double *P_dev, int64_t ldp, double a, double lamb, const double *c_dev);
/* The traces of the objective (optimize.py:374-379) in two launches: dot_p = sum_ij w_p[i] P_p[i, j] Q_p[i, j] for
 * n_pairs <= PK_LCE_MAX_PAIRS blocks [m_p x k_p] (Q_p NULL: ones; w_p NULL: ones; the arrays of pointers and sizes are HOST
 * arrays of n_pairs entries, the pointers in them DEVICE pointers), out_dev[0] = bias + sum_p coef_p dot_p,
 * out_dev[1 + p] = dot_p.  Fixed summation order, no atomics: pair p is cut into pk_lce_dot_blocks(m_p k_p) contiguous
 * ranges whose sums are added in ascending order — equal inputs give equal bits.  work >= pk_lce_dots_work_bytes(). */
#define PK_LCE_MAX_PAIRS 16
int32_t pk_lce_dot_blocks(int64_t n_elems);
int64_t pk_lce_dots_work_bytes(void);
int pk_lce_dots_f64(void *stream, int32_t n_pairs, const double *const *P_dev, const double *const *Q_dev,
                    const double *const *w_dev, const int64_t *m, const int32_t *k, const int64_t *ldp, const int64_t *ldq,
                    const double *coef, double bias, double *out_dev, void *work_dev);
/* E <- max(E, lo) over an [m x k] block: the clamp of LCE's cold-start queries (coldstart/models.py:144) */
int pk_clamp_min_f64(void *stream, int64_t m, int32_t k, double *E_dev, int64_t lde, double lo);

/* ------------------------------------------------------------------------------------------
 * Probabilistic matrix factorisation (csrc/pmf.hip).  Replaces the numba loop `generalized_sgd_sweep`
 * (lib/optimize.py:123-154) as `simple_pmf_sgd` drives it: one SGD sweep over all interactions per epoch.
 * The interactions come in SCHEDULE order (polara_amd/pmf.py: block_schedule): the matrix is cut into B x B blocks, block
 * (i, j) belongs to stratum s = (j - i) mod B, the schedule lists stratum 0's blocks i = 0..B-1, then stratum 1's, ...;
 * block_ptr_dev[s * B + i] .. [s * B + i + 1] are the samples of block i of stratum s.  Two blocks of a stratum share
 * no user and no item, so pk_pmf_epoch_f64 runs them side by side and the result equals the serial sweep over the
 * schedule.  ONE launch per stratum on `stream`; stream order is the only synchronisation between strata (no grid
 * barrier, no cooperative launch, no flag another workgroup waits on).
 *   A block is swept sequentially by one group of w lanes, w = the smallest of 16, 32, 64 that is >= rank; lane c holds
 *   column c, lanes c >= rank hold zeros.  Per sample (m, n, val), exactly optimize.py:129-153 in IEEE fp64 without
 *   contraction, divisions and square roots correctly rounded:
 *     d[c]  = pm[c] * qn[c]                              (0 for c >= rank)
 *     dot   = halving tree: for h = w/2, w/4, .., 1:  d[c] <- d[c] + d[c + h]  (c < h);  dot = d[0]
 *     err   = val - dot;  rl = lambd / row_nnz[m];  cl = lambd / col_nnz[n]
 *     gp    = err * qn - pm * rl;   gq = err * pm - qn * cl            (both from the OLD pm, qn)
 *     adjust (P first, then Q):  none: a = g
 *                                adagrad: S <- S + g * g;                          a = g / sqrt(smoothing + S)
 *                                rmsprop: S <- gamma * S + (1 - gamma) * (g * g);  a = g / sqrt(smoothing + S)
 *     pm <- pm + eta * ap;  qn <- qn + eta * aq;  both rows (and both state rows) are stored
 *   A row (and its state row) stays in registers while consecutive samples of the block share it.
 *   Squared error: every block adds err * err in sample order; one more launch adds the block sums of each stratum in
 *   block order and then the stratum sums in stratum order into sse_dev[0].  No atomics: equal inputs give equal bits.
 * row_nnz_dev / col_nnz_dev: the entry counts per user / item as doubles.  S*_dev: the adjuster's state [n x rank]
 * (NULL for PK_PMF_ADJUST_NONE); the caller zeroes it before every epoch (optimize.py:186-189).
 * work_dev: pk_pmf_work_doubles(blocks) doubles.  The kernel trusts the plan (indices in range, block_ptr ascending). */
#define PK_PMF_ADJUST_NONE 0
#define PK_PMF_ADJUST_ADAGRAD 1
#define PK_PMF_ADJUST_RMSPROP 2
#define PK_PMF_MAX_BLOCKS 4096
int32_t pk_pmf_max_rank(void);
int64_t pk_pmf_work_doubles(int32_t blocks);
int pk_pmf_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, const int64_t *block_ptr_dev,
                     const int32_t *users_dev, const int32_t *items_dev, const double *vals_dev, double *P_dev, int64_t ldp,
                     double *Q_dev, int64_t ldq, const double *row_nnz_dev, const double *col_nnz_dev, double eta,
                     double lambd, int32_t adjust, double *SP_dev, int64_t ldsp, double *SQ_dev, int64_t ldsq, double gamma,
                     double smoothing, double *work_dev, double *sse_dev);

/* ------------------------------------------------------------------------------------------
 * Kernelized probabilistic matrix factorisation (csrc/kpmf.hip).  Replaces `generalized_sgd_sweep` as
 * `kernelized_pmf_sgd` drives it (lib/optimize.py:258-301: the transform `sparse_kernel_update`).  Everything is PMF
 * above — schedule, lane groups, halving tree, lambdas, adjusters, squared error — except the two gradients:
 *     off_p = (+0.0 + Ku[e1] * X(j1)) + Ku[e2] * X(j2) + ...   over the stored entries e of row m of Ku WITHOUT its diagonal,
 *                                                             in storage order, every product and every sum rounded
 *     X(j)  = P[j]       (live)  if user_part[j] == I          (I, J: the user part and the item part of the sample's block;
 *           = P_snap[j]          otherwise                      block i of stratum s has I = i, J = (i + s) mod B)
 *     kp    = off_p + du[m] * (pm + pm)                        du[m]: the diagonal of row m (0.0 when none is stored); the
 *                                                             reference's diagonal term is value * (P[m] + pm)
 *     gp    = err * qn - kp * rl
 *     kq, gq likewise with Ki, item_part, J, Q, Q_snap, di and cl.
 * P_snap / Q_snap [n x rank, leading dimensions of their own] hold P and Q as they stood when the stratum began: the entry
 * copies both blocks before the first stratum and after every stratum (so they equal P and Q when the epoch ends).  Rows of
 * a block's own parts are written by that block alone during the stratum and the block is swept serially, so their live
 * value is well defined; every other row comes from the snapshot, so no block reads what another is writing.  With B = 1
 * every row is live and the sweep is the reference's; with B > 1 the neighbour rows of the regulariser (and nothing else)
 * are stale by at most one stratum.  off_p is computed once per run of samples that share the user.
 * k*_ptr_dev [n + 1] int64, k*_idx_dev int32 (sorted within a row, no diagonal), k*_val_dev, k*_diag_dev [n] fp64;
 * *_part_dev [n] int32: the part of every user / item in the schedule.  The kernel trusts the plan and the kernel matrices
 * (indices in range). */
int pk_kpmf_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, int64_t n_users, int64_t n_items,
                      const int64_t *block_ptr_dev, const int32_t *users_dev, const int32_t *items_dev,
                      const double *vals_dev, double *P_dev, int64_t ldp, double *Q_dev, int64_t ldq,
                      const double *row_nnz_dev, const double *col_nnz_dev, const int32_t *user_part_dev,
                      const int32_t *item_part_dev, const int64_t *ku_ptr_dev, const int32_t *ku_idx_dev,
                      const double *ku_val_dev, const double *ku_diag_dev, const int64_t *ki_ptr_dev,
                      const int32_t *ki_idx_dev, const double *ki_val_dev, const double *ki_diag_dev,
                      double *P_snap_dev, int64_t ldps, double *Q_snap_dev, int64_t ldqs, double eta, double lambd,
                      int32_t adjust, double *SP_dev, int64_t ldsp, double *SQ_dev, int64_t ldsq, double gamma,
                      double smoothing, double *work_dev, double *sse_dev);

/* ------------------------------------------------------------------------------------------
 * Bayesian personalised ranking (csrc/bpr.hip): LearnBPR (Rendle et al., 2009) with rank k plus an item bias, fp64.
 * P [n_users x (k + 1)]: column k is the constant 1 and is never written.  Q [n_items x (k + 1)]: column k is the bias.
 * The positives are the stored entries of the training CSR (entry e = its position in storage), in the SCHEDULE order of
 * PMF above — with the items cut into parts along the epoch's item order pi (polara_amd/bpr.py): part c of the items is
 * item_order[item_ptr[c] .. item_ptr[c + 1]], and item_part[i] is the part of item i.  perm[p] is the entry at position p.
 *   Negatives (pk_bpr_draw_negatives, one thread per position):  mix64 = the splitmix64 output function,
 *     h = mix64(seed * 2^32 + epoch);  for t = 0 .. PK_BPR_DRAWS - 1:
 *       w = mix64(h + 4 * e + t) >> 32;   x = (w * n_c) >> 32  (64-bit; n_c = the size of the positive's item part c);
 *       j = item_order[item_ptr[c] + x];  the first j that is not in row u of the CSR (binary search on its sorted
 *       columns) is the negative.  neg[p] = -1 when all draws are seen items: the sample is skipped.
 *   A block is swept sequentially by one group of w lanes, w = the smallest of 16, 32, 64 that is >= k + 1; lane c holds
 *   column c.  Per sample (u, i, j) in IEEE fp64 without contraction, the division correctly rounded:
 *     d[c]  = Qi[c] - Qj[c]                                     (c = 0..k; 0 beyond)
 *     x     = halving tree over P[u][c] * d[c] as in PMF above
 *     z     = sigm(x) = 1 / (1 + exp(x)), by the sequence below
 *     P[u][c] <- P[u][c] + lr * (z * d[c] - reg * P[u][c])      (c < k)
 *     Qi[c]   <- Qi[c] + lr * (z * P_old[u][c] - reg * Qi[c])   (c <= k)
 *     Qj[c]   <- Qj[c] - lr * (z * P_old[u][c] + reg * Qj[c])   (c <= k)
 *     correct += (x > 0);  trained += 1.   A skipped sample loads and stores nothing and counts as skipped.
 *   A row stays in registers while the next sample of the block uses it again: the user row, and either item row in
 *   either role.  Counts are 64-bit integers per block, added per stratum and then per epoch: counts_dev[0..2] =
 *   trained, skipped, correct.  No atomics.
 *   sigm(x):  a = -|x|, raised to -750 when below (a NaN stays);  n = floor(a * 0x1.71547652b82fep+0 + 0.5);
 *     r = (a - n * 0x1.62e42feep-1) - n * 0x1.a39ef35793c76p-33;  T = Horner form of sum_{m = 0..13} r^m / m! with the
 *     doubles nearest to 1 / m!;  e = ldexp(T, n);  sigm = 1 / (1 + e) for x <= 0 (and NaN), e / (1 + e) for x > 0.
 *     pk_bpr_sigmoid_f64 is this function alone, elementwise.
 * work_dev: pk_bpr_work_bytes(blocks) bytes.  The kernels trust the plan (indices in range, block_ptr ascending). */
#define PK_BPR_DRAWS 4
int32_t pk_bpr_max_rank(void);
int64_t pk_bpr_work_bytes(int32_t blocks);
int pk_bpr_sigmoid_f64(void *stream, int64_t n, const double *x_dev, double *out_dev);
int pk_bpr_draw_negatives(void *stream, int64_t nnz, int64_t n_users, int64_t n_items, int32_t blocks,
                          const int32_t *users_dev, const int32_t *items_dev, const int64_t *perm_dev,
                          const int32_t *item_order_dev, const int32_t *item_part_dev, const int64_t *item_ptr_dev,
                          const int64_t *indptr_dev, const int32_t *indices_dev, uint32_t seed, uint32_t epoch,
                          int32_t *neg_dev);
int pk_bpr_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, const int64_t *block_ptr_dev,
                     const int32_t *users_dev, const int32_t *items_dev, const int32_t *neg_dev, double *P_dev, int64_t ldp,
                     double *Q_dev, int64_t ldq, double learning_rate, double regularization, void *work_dev,
                     int64_t *counts_dev);

/* ------------------------------------------------------------------------------------------
 * LightFM with the WARP loss (csrc/warp.hip; polara_amd/warp.py): rank k plus a bias, per-parameter adagrad, fp64, C = k + 1.
 * P [n_users x C]: column k is the constant 1 and is never written.  E_id [n_items x C]: the items' identity embeddings,
 * column k the bias.  E_lab [n_labels x C]: the label embeddings, column k the label's bias.  AP, AE, AL: the adagrad state
 * of the three blocks, same shapes, 1 at build start and kept over the epochs (column k of AP is never touched).
 * Item features: item i with m_i labels has a[i] = 1 / (1 + m_i); F_lab = diag(a) one_hot [n_items x n_labels], given as CSR
 * (row_*: labels ascending within an item) and CSC (col_*: items ascending within a label).  The representation of item i is
 *     q_i = a[i] * E_id[i] + S[i],   S[i] = (+0.0 + F[i,l1] * E_lab[l1]) + F[i,l2] * E_lab[l2] + ...  (storage order)
 * Without features (a_dev == NULL) q_i = E_id[i]: no multiplication, no S, no G, no label launches.
 * The positives, the schedule, the item order, the parts and perm are BPR's above.
 *   Candidates (pk_warp_draw_candidates, one thread per position and draw):  D = max_sampled, 1 <= D <= PK_WARP_MAX_SAMPLED,
 *     h = mix64(seed * 2^32 + epoch);  for t = 0 .. D - 1:  w = mix64(h + 64 * e + t) >> 32;  x = (w * n_c) >> 32;
 *     j = item_order[item_ptr[c] + x]  (c, n_c: the positive's item part and its size);  cand[p * D + t] = j, or -1 when j lies
 *     in row u of the CSR.  A -1 counts as a draw and is passed over.
 *   Loss table (host, NumPy fp64, D doubles):  table[t] = min(10, log(max(1, floor((n_items - 1) / (t + 1))))).
 *   One epoch (pk_warp_epoch_f64), per stratum s in stream order:
 *     1. with features: S = F_lab E_lab over all items as above, and G [n_items x C] is cleared  (one launch)
 *     2. the sweep (one launch): a block is swept sequentially by one group of w lanes, w = the smallest of 16, 32, 64 that is
 *        >= C; lane c holds column c.  Per sample (u, i) in IEEE fp64 without contraction, division and square root
 *        correctly rounded, tree = the halving tree of PMF above over C columns:
 *          x_pos = tree(P[u] * q_i)
 *          for t = 0 .. D - 1:  j = cand[t];  draws += 1;  if j < 0: continue
 *              x_neg = tree(P[u] * q_j);   if not (x_neg > x_pos - 1): continue
 *              L   = table[t]
 *              g_u = L * (q_j - q_i)  (c < k);   g_i = -(L * P_old[u])  (c <= k);   g_j = L * P_old[u]  (c <= k)
 *              adagrad per element:  step = lr / sqrt(A);  x <- x - step * g;  A <- A + g * g
 *                on P[u] with g_u (state AP[u]), on E_id[i] with a[i] * g_i (AE[i]), on E_id[j] with a[j] * g_j (AE[j]);
 *                without features the gradients of E_id are g_i and g_j themselves
 *              with features:  G[i] <- G[i] + g_i;  G[j] <- G[j] + g_j
 *              trained += 1;  stop
 *          no violator: quiet += 1, nothing is stored.
 *        q_i and q_j are formed from the LIVE identity rows (a row stays in registers while the next sample of the block
 *        uses it again) and from the S of step 1.
 *     3. with features, the label step (one launch; pk_warp_label_step_f64 is this step alone, followed by clearing G):
 *          g_l = (+0.0 + F[i1,l] * G[i1]) + F[i2,l] * G[i2] + ...  over the items of label l ascending, per column c <= k;
 *          the adagrad step above on E_lab[l] with g_l (state AL[l]).
 *   After the last stratum G is cleared (with features) and the 64-bit block counters are added per stratum and then per
 *   epoch: counts_dev[0..2] = trained, quiet, draws.  No atomics, no flags: E_lab is read-only while a stratum runs, the rows
 *   of P, E_id, their states and G that a block writes are its own, and stream order separates the launches.  The label
 *   embeddings therefore take `blocks` steps per epoch, each on one stratum's summed gradient.
 * pk_warp_label_image_f64: S alone (step 1 without clearing G).
 * work_dev: pk_warp_work_bytes(blocks) bytes.  The kernels trust the plan, the candidates and the feature matrices (indices
 * in range, pointers ascending). */
#define PK_WARP_MAX_SAMPLED 64
int32_t pk_warp_max_rank(void);
int64_t pk_warp_work_bytes(int32_t blocks);
int pk_warp_draw_candidates(void *stream, int64_t nnz, int64_t n_users, int64_t n_items, int32_t blocks, int32_t max_sampled,
                            const int32_t *users_dev, const int32_t *items_dev, const int64_t *perm_dev,
                            const int32_t *item_order_dev, const int32_t *item_part_dev, const int64_t *item_ptr_dev,
                            const int64_t *indptr_dev, const int32_t *indices_dev, uint32_t seed, uint32_t epoch,
                            int32_t *cand_dev);
int pk_warp_label_image_f64(void *stream, int32_t rank, int64_t n_items, int64_t n_labels, const int64_t *row_ptr_dev,
                            const int32_t *row_idx_dev, const double *row_val_dev, const double *L_dev, int64_t ldl,
                            double *S_dev, int64_t lds);
int pk_warp_label_step_f64(void *stream, int32_t rank, int64_t n_items, int64_t n_labels, const int64_t *col_ptr_dev,
                           const int32_t *col_idx_dev, const double *col_val_dev, double *G_dev, int64_t ldg, double *L_dev,
                           int64_t ldl, double *AL_dev, int64_t ldal, double learning_rate);
int pk_warp_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, int64_t n_items, int64_t n_labels,
                      int32_t max_sampled, const int64_t *block_ptr_dev, const int32_t *users_dev, const int32_t *items_dev,
                      const int32_t *cand_dev, const double *loss_table_dev, double *P_dev, int64_t ldp, double *E_dev,
                      int64_t lde, double *AP_dev, int64_t ldap, double *AE_dev, int64_t ldae, double learning_rate,
                      const double *a_dev, const int64_t *row_ptr_dev, const int32_t *row_idx_dev, const double *row_val_dev,
                      const int64_t *col_ptr_dev, const int32_t *col_idx_dev, const double *col_val_dev, double *L_dev,
                      int64_t ldl, double *AL_dev, int64_t ldal, double *S_dev, int64_t lds, double *G_dev, int64_t ldg,
                      void *work_dev, int64_t *counts_dev);

/* ------------------------------------------------------------------------------------------
 * Factorisation model with side features (csrc/fm.hip; polara_amd/fm.py): rating regression with a global mean mu, user and
 * item biases, linear weights of the side features and factorised interactions, fp64.  Rank k, C = k + 2 columns:
 *     P  [n_users   x C]  user identity rows:  factors | bias          | 1  (never written)
 *     LU [n_ulabels x C]  user label rows:     factors | linear weight | 0  (never written)
 *     E  [n_items   x C]  item identity rows:  factors | 1  (never written) | bias
 *     LI [n_ilabels x C]  item label rows:     factors | 0  (never written) | linear weight
 * Features of a side: weights a [n_rows] and F [n_rows x n_labels] as CSR (row_*: labels ascending within a row) and CSC
 * (col_*: rows ascending within a label), any values.  Representations and prediction:
 *     pt_u = aU[u] * P[u] + SU[u],   SU[u] = (+0.0 + FU[u,l1] * LU[l1]) + FU[u,l2] * LU[l2] + ...   (storage order)
 *     qt_i = aI[i] * E[i] + SI[i],   SI likewise;   a side without features (a*_dev == NULL) has pt_u = P[u] (qt_i = E[i]): no
 *     multiplication, no S, no G, no label launches.
 *     yhat(u, i) = mu + sum_c pt_u[c] * qt_i[c]
 * Interactions inside one side (identity x own labels, label x label) are not modelled.
 * The interactions, the schedule and the lane groups are PMF's above (w = the smallest of 16, 32, 64 that is >= C).
 * Step rule (x the parameter, g its gradient, s its state; state blocks have the shapes of their parameters, start at 0 and are
 * NOT cleared between epochs):   x <- x - step * adj(g, s)   with adj the adjusters of PMF above (NONE: adj = g).
 * lam(c) = regularization for c < k, linear_regularization for the bias / linear-weight column.
 *   One epoch (pk_fm_epoch_f64), per stratum in stream order:
 *     1. per side with features (one launch each): S = F L as above and G [n_rows x (C + 1)] is cleared
 *     2. the sweep (one launch).  Per sample (u, i, r) in IEEE fp64 without contraction, tree = PMF's halving tree over C columns:
 *          pt, qt from the LIVE identity rows and the S of step 1
 *          err = (mu + tree(pt * qt)) - r
 *          eq = err * qt;   ep = err * pt                               (per column, both from the rows before the update)
 *          gp = aU[u] * eq + lam(c) * P[u][c]    (without user features: eq + lam(c) * P[u][c])     for c <= k
 *          gq = aI[i] * ep + lam(c) * E[i][c]    (without item features: ep + lam(c) * E[i][c])     for c < k and c = k + 1
 *          the step rule on P[u] with gp (state SP[u]) and on E[i] with gq (state SE[i]), those columns only
 *          with user features:  GU[u][c] <- GU[u][c] + eq  (c < C);  GU[u][C] <- GU[u][C] + 1
 *          with item features:  GI[i][c] <- GI[i][c] + ep  (c < C);  GI[i][C] <- GI[i][C] + 1
 *          the block's squared error += err * err   (reduced as PMF's into sse_dev[0])
 *        A row (with its state row, its row of G and its count) stays in registers while consecutive samples share it.
 *     3. per side with features, the label step (one launch each; pk_fm_label_step_f64 is this step alone, followed by clearing
 *        G).  Per label l and column c — c = k (user side) or k + 1 (item side), and c < k when label_factors != 0:
 *          g = (+0.0 + F[r1,l] * G[r1][c]) + F[r2,l] * G[r2][c] + ...;   N = (+0.0 + G[r1][C]) + G[r2][C] + ...   (rows ascending)
 *          N == 0 (no row of the label was sampled in the stratum): nothing is done
 *          g <- g + (lam(c) * N) * L[l][c];   the step rule on L[l][c] with g (state SL[l][c])
 *   After the last stratum G is cleared.  No atomics, no flags: the label rows are read-only while a stratum runs, the rows
 *   of P, E, their states and G that a block writes are its own, and stream order separates the launches.  The label rows
 *   therefore take `blocks` steps per epoch, each on one stratum's summed gradient.
 * pk_fm_label_image_f64: S alone (step 1 without clearing G).  item_side: 0 for user labels, 1 for item labels.
 * work_dev: pk_pmf_work_doubles(blocks) doubles.  The kernels trust the plan and the feature matrices (indices in range,
 * pointers ascending). */
int32_t pk_fm_max_rank(void);
int pk_fm_label_image_f64(void *stream, int32_t rank, int64_t n_rows, int64_t n_labels, const int64_t *row_ptr_dev,
                          const int32_t *row_idx_dev, const double *row_val_dev, const double *L_dev, int64_t ldl,
                          double *S_dev, int64_t lds);
int pk_fm_label_step_f64(void *stream, int32_t rank, int32_t item_side, int32_t label_factors, int64_t n_rows,
                         int64_t n_labels, const int64_t *col_ptr_dev, const int32_t *col_idx_dev,
                         const double *col_val_dev, double *G_dev, int64_t ldg, double *L_dev, int64_t ldl, double *SL_dev,
                         int64_t ldsl, double step, double regularization, double linear_regularization, int32_t adjust,
                         double gamma, double smoothing);
int pk_fm_epoch_f64(void *stream, int32_t blocks, int32_t rank, int64_t nnz, int64_t n_users, int64_t n_items,
                    const int64_t *block_ptr_dev, const int32_t *users_dev, const int32_t *items_dev, const double *vals_dev,
                    double mean, double *P_dev, int64_t ldp, double *E_dev, int64_t lde, double step, double regularization,
                    double linear_regularization, int32_t adjust, double *SP_dev, int64_t ldsp, double *SE_dev, int64_t ldse,
                    double gamma, double smoothing, int32_t label_factors,
                    int64_t n_ulabels, const double *au_dev, const int64_t *urow_ptr_dev, const int32_t *urow_idx_dev,
                    const double *urow_val_dev, const int64_t *ucol_ptr_dev, const int32_t *ucol_idx_dev,
                    const double *ucol_val_dev, double *LU_dev, int64_t ldlu, double *SLU_dev, int64_t ldslu, double *SU_dev,
                    int64_t ldsu, double *GU_dev, int64_t ldgu,
                    int64_t n_ilabels, const double *ai_dev, const int64_t *irow_ptr_dev, const int32_t *irow_idx_dev,
                    const double *irow_val_dev, const int64_t *icol_ptr_dev, const int32_t *icol_idx_dev,
                    const double *icol_val_dev, double *LI_dev, int64_t ldli, double *SLI_dev, int64_t ldsli, double *SI_dev,
                    int64_t ldsi, double *GI_dev, int64_t ldgi, double *work_dev, double *sse_dev);

/* ------------------------------------------------------------------------------------------
 * Implicit ALS (csrc/ials.hip): the alternating least squares of Hu, Koren and Volinsky for a CSR of confidences C
 * [n_rows x n_cols] (fp64 values, int64 row pointers, int32 column ids).  One half-step fixes Y [n_cols x rank] and solves
 * for every row u
 *     A_u = G + lambda I + sum_{i in row u} (c_ui - 1) y_i y_i^T,    b_u = sum_i c_ui y_i,    x_u = A_u^-1 b_u
 * with G = Y^T Y from the caller (pk_gram_f64).  One workgroup per row, taken in the order row_order_dev lists them (a
 * permutation of 0 .. n_rows - 1, longest rows first; NULL: ascending).  Everything is fp64.  The sum over a row runs in
 * storage order in groups of four (v_mfma_f64_16x16x4_f64 over the lower-triangular 16 x 16 tiles, accumulators started from
 * G + lambda I); b_u is summed entry after entry in storage order; A_u is factored by a right-looking Cholesky in LDS and
 * solved by forward and back substitution.  The order of every summation depends on the row alone: equal inputs give equal
 * bits, whatever the row order.  No atomics.  An empty row gives x_u = 0 exactly.
 * info_dev: two int32 — the number of rows with a pivot that is not > 0 (NaN included) and the first such row (-1: none);
 * the rows of X of those are written as zeros.  work_dev: pk_ials_work_bytes(n_rows, rank) bytes.  Column ids outside
 * 0 .. n_cols - 1 contribute nothing.
 * pk_ials_loss_nz_f64: out_dev[0] = sum over stored entries of c (1 - s)^2 - s^2 with s = x_u . y_i — the sparse term of
 *     sum_all-pairs w (p - s)^2 + lambda (|X|^2 + |Y|^2) = tr(X^T X Y^T Y) + sparse term + lambda (tr X^T X + tr Y^T Y);
 * one wave per row, terms added in storage order, row sums added in a fixed order. */
int32_t pk_ials_max_rank(void);
int64_t pk_ials_work_bytes(int64_t n_rows, int32_t rank);
int pk_ials_half_step_f64(void *stream, int64_t n_rows, int64_t n_cols, int32_t rank, const int64_t *indptr_dev,
                          const int32_t *indices_dev, const double *conf_dev, const int32_t *row_order_dev, const double *Y_dev,
                          int64_t ldy, const double *G_dev, int64_t ldg, double lambda, double *X_dev, int64_t ldx,
                          int32_t *info_dev, void *work_dev);
int pk_ials_loss_nz_f64(void *stream, int64_t n_rows, int64_t n_cols, int32_t rank, const int64_t *indptr_dev,
                        const int32_t *indices_dev, const double *conf_dev, const double *X_dev, int64_t ldx, const double *Y_dev,
                        int64_t ldy, double *out_dev, void *work_dev);

/* ------------------------------------------------------------------------------------------
 * iALS++ (csrc/ialspp.hip): the block-subspace solver of Rendle, Krichene, Zhang and Koren for the objective of implicit ALS,
 * ranks 1 .. pk_ialspp_max_rank() (2048).  E [nnz] caches e = x_u . y_i for the stored entries of C in storage order.
 * pk_ialspp_predict_f64: E from X [n_rows x rank] and Y [n_cols x rank]; one wave per row, a fixed order of summation.
 * pk_ialspp_block_step_f64: with pi = [p0, min(p0 + block_size, rank)), block_size 16, 32 or 64, for every row u
 *     g = r_u + lambda_u x_pi + sum_i ((c_i - 1) e_i - c_i) y_{i,pi},    H = G[pi,pi] + lambda_u I + sum_i (c_i - 1) y_{i,pi} y_{i,pi}^T
 *     delta = H^-1 g (Cholesky, fp64);    x_pi -= delta;    e_i -= y_{i,pi} . delta          — in place on X and E
 * with R [n_rows x |pi|] = X G[:,pi] formed by the caller from the X the step starts from, G = Y^T Y [rank x rank], lambda_u =
 * lambda_rows_dev[u] when that pointer is not null, else lambda.  Rows are taken in row_order_dev (int32 permutation; null:
 * 0, 1, ..); the order of every summation depends on the row alone: equal inputs give equal bits, whatever the row order.  No
 * atomics.  An empty row gets x_pi = 0 exactly.  info_dev: two int32 — the number of rows with a pivot that is not > 0 (NaN
 * included) and the first such row (-1: none); x_pi and e of those rows are left as they were.  work_dev:
 * pk_ialspp_work_bytes(n_rows, block_size) bytes.  Column ids outside 0 .. n_cols - 1 contribute nothing (predict: e = 0). */
int32_t pk_ialspp_max_rank(void);
int64_t pk_ialspp_work_bytes(int64_t n_rows, int32_t block_size);
int pk_ialspp_block_step_f64(void *stream, int64_t n_rows, int64_t n_cols, int32_t rank, int32_t p0, int32_t block_size,
                             const int64_t *indptr_dev, const int32_t *indices_dev, const double *conf_dev,
                             const int32_t *row_order_dev, const double *Y_dev, int64_t ldy, const double *G_dev, int64_t ldg,
                             double lambda, const double *lambda_rows_dev, const double *R_dev, int64_t ldr, double *X_dev,
                             int64_t ldx, double *E_dev, int32_t *info_dev, void *work_dev);
int pk_ialspp_predict_f64(void *stream, int64_t n_rows, int64_t n_cols, int32_t rank, const int64_t *indptr_dev,
                          const int32_t *indices_dev, const double *X_dev, int64_t ldx, const double *Y_dev, int64_t ldy,
                          double *E_dev);

/* ------------------------------------------------------------------------------------------
 * Logistic matrix factorisation (csrc/lmf.hip; polara_amd/lmf.py): Johnson (2014) in the shape the `implicit` package trains it
 * — rank k plus a bias on either side, per-parameter AdaGrad, sampled negatives —, fp64.  Blocks carry K = k + 2 columns: the user
 * block [factors | bias | 1], the item block [factors | 1 | bias], so that their product are the logits (and the scores).
 * One half-step fixes Y [n_cols x K] and moves, for a CSR of confidences C [n_rows x n_cols] (fp64 values, int64 row pointers,
 * int32 column ids), every row u of X [n_rows x K] with n > 0 stored entries (confidences c_q in storage order), together with
 * its AdaGrad state A [n_rows x K] (zeros at build start, kept over the epochs):
 *   negatives:  m = min(n_cols, n * neg_prop);  neg_ptr = the exclusive prefix sum of m over the rows (int64 [n_rows + 1]);
 *     h = mix64(seed * 2^32 + round)  (mix64 = the splitmix64 output function, the key of the BPR stream above);
 *     negative t = 0 .. m - 1 is column ((mix64(h + neg_ptr[u] + t) >> 32) * n_cols) >> 32  (64-bit) — uniform over ALL
 *     columns, with replacement, the row's own entries included (the sampled term estimates the sum over all items);
 *   the sample list q = 0 .. n + m - 1: the positives in storage order, then the negatives in draw order; y_q its row of Y;
 *   in IEEE fp64 without contraction, every product and sum rounded on its own, sqrt and division correctly rounded:
 *     s_q  = (..((x_0 * y_q0) + x_1 * y_q1) + ..) + x_{K-1} * y_q,K-1           (x = the row as it was before the step)
 *     g_q  = c_q * sigm(s_q) for a positive,  -sigm(-s_q) for a negative         (sigm(x) = 1 / (1 + exp(x)): the BPR sequence)
 *     D_c  = chain_0 + chain_1 + .. + chain_{PK_LMF_CHAINS - 1}  (left to right),  chain_j = 0 + sum over q = j mod PK_LMF_CHAINS,
 *            ascending, of g_q * y_qc  (left to right)
 *     d_c  = D_c - reg * x_c;   a_c = A[u][c] + d_c * d_c;   A[u][c] <- a_c;   X[u][c] <- x_c + (lr / sqrt(1e-6 + a_c)) * d_c
 *   for every column c but pinned_col (the constant 1: K - 1 of the user block, K - 2 of the item block; -1: none), which is
 *   touched neither in X nor in A.  An empty row is not touched at all.  No row is refused: a NaN propagates.
 * One workgroup per row, taken in the order row_order_dev lists them (a permutation of 0 .. n_rows - 1, longest rows first;
 * NULL: ascending); the order of every summation depends on the row alone: equal inputs give equal bits, whatever the row order.
 * No atomics; no sample array exists.  Column ids outside 0 .. n_cols - 1 read a row of zeros.  pk_lmf_max_rank() = 126 (K <= 128).
 * pk_lmf_draw_negatives: out_dev[neg_ptr[u] + t] = negative t of row u, through the half-step's own draw function (int32
 * [neg_ptr[n_rows]]); a row whose neg_ptr does not span min(n_cols, n * neg_prop) is skipped.  pk_lmf_chains() = PK_LMF_CHAINS. */
#ifndef PK_LMF_CHAINS
#define PK_LMF_CHAINS 4
#endif
int32_t pk_lmf_max_rank(void);
int32_t pk_lmf_chains(void);
int pk_lmf_half_step_f64(void *stream, int64_t n_rows, int64_t n_cols, int32_t K, const int64_t *indptr_dev,
                         const int32_t *indices_dev, const double *conf_dev, const int32_t *row_order_dev,
                         const int64_t *neg_ptr_dev, uint32_t seed, uint32_t round, int32_t pinned_col, int32_t neg_prop,
                         const double *Y_dev, int64_t ldy, double learning_rate, double regularization, double *X_dev,
                         int64_t ldx, double *A_dev, int64_t lda);
int pk_lmf_draw_negatives(void *stream, int64_t n_rows, int64_t n_cols, const int64_t *indptr_dev,
                          const int64_t *neg_ptr_dev, int32_t neg_prop, uint32_t seed, uint32_t round, int32_t *out_dev);

/* ------------------------------------------------------------------------------------------
 * K5.  Sparse tensor-times-matrix (CoFFee / HOOI).
 * Replaces numba `dttm_seq` / `dttm_par` (lib/sparse.py:203-234) called from `ttm3d_seq`
 * (lib/tensor.py:7-19):  res[i0, j, k] += val * u[i1, j] * v[i2, k].
 * nnz are pre-sorted by the output mode by the host layer; tasks as in pk_spmm_csr_ex, with
 * idx1/idx2 the two contracted-mode indices of every nnz and `vals` optional (NULL = ones,
 * data.py:805).  res is [n0 x (ra*rb)] row-major, ra * rb <= 1024.
 * EVERY row of u and of v must be finite, rows that no entry references included: the padded steps of a task's
 * last chunk multiply u[0, :] and v[0, :] by the value 0 instead of branching.
 * ------------------------------------------------------------------------------------------ */
int pk_ttm_f64(void *stream,
               int64_t n_tasks, const int32_t *task_row_dev, const int64_t *task_begin_dev,
               const int64_t *task_end_dev, const int32_t *task_slot_dev,
               int64_t n_long, const int32_t *long_row_dev, const int32_t *long_slot_begin_dev,
               const int32_t *long_slot_end_dev,
               const int32_t *idx1_dev, const int32_t *idx2_dev, const double *vals_dev,
               const double *u_dev, int64_t ldu, int32_t ra, const double *v_dev, int64_t ldv_, int32_t rb,
               double *res_dev, int64_t ldr, double *partial_dev);
/* CoffeeModel.predict_feedback (models.py:1068-1091): for each of n holdout (user, item) pairs the index of the feedback
 * level f with the largest reconstructed score  sum_abc core[a, b, c] u[user, a] v[item, b] w[f, c]  (first maximum, as
 * np.argmax).  u [n_users x r0], v [n_items x r1], w [L x r2] row-major fp64, core [r0 x r1 x r2] C-ordered, r2 <= 16.
 * pred_dev int64[n]; scores_dev [n x L] or NULL. */
int pk_tucker_predict_f64(void *stream, int64_t n, const int64_t *users_dev, const int64_t *items_dev,
                          const double *u_dev, int64_t ldu, const double *v_dev, int64_t ldv_, const double *w_dev,
                          int64_t ldw, const double *core_dev, int32_t r0, int32_t r1, int32_t r2, int32_t L,
                          int64_t *pred_dev, double *scores_dev);


/* ------------------------------------------------------------------------------------------
 * Coarse entry points: what a host in ANY language binds to replace the two hot calls of the
 * reference without re-writing the solver or the scoring pipeline — `SVDModel.build` (models.py:835-855: svds of the
 * training matrix) and `get_recommendations` (models.py:391-405 with 857-861, 494-519, 488-491).  Host pointers in,
 * caller-allocated HOST buffers out; device memory lives behind opaque handles owned by the library; every call
 * on one context is serialised by a mutex inside it (the reference's thread pool, models.py:374-382, is safe),
 * distinct contexts are independent; no torch, no Python.  Errors: negative return code + pk_ctx_error(ctx).
 * (The kernel-granular functions above stay the interface of polara_amd's own Python layer, which keeps its device
 * arrays in torch tensors and shards over RCCL; the coarse calls are single-GPU.)
 * ------------------------------------------------------------------------------------------ */
typedef struct pk_ctx pk_ctx;   /* one device + one stream + one mutex */
typedef struct pk_mat pk_mat;   /* a CSR matrix resident on the device with its task plan (and, lazily, its user-blocked transpose) */
typedef struct pk_build_stats {
    int32_t outer;              /* outer iterations (Rayleigh-Ritz + filter) */
    int32_t gramian_steps;      /* applications of A^T A to the block */
    int32_t block;              /* block width */
    int32_t converged;          /* 1 = every leading pair met tol * sigma_1^2 */
    double final_rel_residual;  /* worst ||A^T A v - sigma^2 v|| / sigma_1^2 of the leading k pairs */
} pk_build_stats;
int pk_ctx_create(int32_t device, pk_ctx **ctx_out);
void pk_ctx_destroy(pk_ctx *ctx);
const char *pk_ctx_error(pk_ctx *ctx);
/* host CSR (indptr int64[n_rows + 1], indices int32, values f32 | f64) -> device matrix.  The rows of a TRAINING matrix
 * are users (models.py:160-177); for pk_score_topk the rows are the test users' known interactions with explicit
 * zeros kept — they contribute nothing to the fold-in but still count as seen (models.py:198-203, 494-519). */
int pk_mat_from_csr(pk_ctx *ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *indptr_host,
                    const int32_t *indices_host, const void *values_host, int32_t val_kind, pk_mat **mat_out);
/* host COO triplets, any order, duplicates summed (what `coo_matrix(...).tocsr()` does, models.py:172-175); entry i has
 * row rows_host[i * idx_stride], column cols_host[i * idx_stride] (idx_stride = 2 with cols = rows + 1 reads the
 * interleaved [nnz x 2] index array of `to_coo`, data.py:794-817, as it is) */
int pk_mat_from_coo(pk_ctx *ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *rows_host,
                    const int64_t *cols_host, int64_t idx_stride, const void *values_host, int32_t val_kind,
                    pk_mat **mat_out);
void pk_mat_free(pk_ctx *ctx, pk_mat *mat);
int64_t pk_mat_nnz(const pk_mat *mat);   /* stored entries (after duplicate sums) */
/* Top-k singular triplets of A (models.py:841-853): sigma_out[k] descending, V_out[n_cols * k] COLUMN-major (the
 * F-ordered `vh.T` of models.py:849: column j = right singular vector j), U_out[n_rows * k] column-major or NULL
 * (`return_factors`, models.py:841,853).  block = 0: k + max(14, 0.28 k) rounded up to 8; tol <= 0: 1e-12 (relative to
 * sigma_1^2, on ||A^T A v - sigma^2 v||); max_outer <= 0: 200.  Returns PK_E_NOCONV (with the best available factors
 * written) when it stops unconverged — the reference's ARPACK raises there. */
int pk_svd_build(pk_ctx *ctx, pk_mat *A, int32_t k, int32_t block, double tol, int32_t max_outer, uint64_t seed,
                 double *sigma_out, double *V_out, double *U_out, pk_build_stats *stats_out);
/* The same build with the USERS sharded over `comm->world` ranks — one process (or thread) and one pk_ctx per GPU, the
 * multi-device form of the coarse API (SURVEY 8b sketched `pk_ctx_create(device_ids, n_dev)`; with one process per GPU
 * the devices meet through a communicator instead).  `A_local` holds this rank's rows (users) of the training matrix,
 * all n_cols columns.  What is exchanged is exactly north_star's "all-reduce only for the Gramian step": after every
 * Z = A_p^T (A_p X) the [n_cols x l] block is summed over ranks, and so is the l x l Rayleigh-Ritz matrix (A_p X)^T (A_p X);
 * everything on the item side (orthonormalisation, filter recurrences, eigen-decompositions, locking decisions) is
 * computed identically on every rank from all-reduced data and the same seed.  sigma_out / V_out are global and equal on
 * all ranks; U_out (or NULL) holds this rank's rows.  Scoring needs no collective: every rank calls pk_score_topk /
 * pk_serving_* on its own users with the replicated V.
 * The library does not link a collective library: the host passes its communicator as a callback — with RCCL
 *     int ar(void *user, void *buf, int64_t n, void *stream) {
 *         return ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, (ncclComm_t)user, (hipStream_t)stream) == ncclSuccess ? 0 : -1; }
 * `stream` is the HIP stream the call must be ordered on (enqueue there, or block until done): the context's stream, or
 * — when the exchange of a Gramian product is long enough to be worth hiding (modelled all-reduce >= 0.4 ms; context option
 * "dist_overlap") — a side stream of the library for the FIRST of the product's two column panels, whose sum then travels
 * while the second panel is computed (the same rule and the same two panels as polara_amd/solver.py::ItemRows.product).
 * Every rank issues its calls in the same order. */
typedef struct pk_comm {
    int32_t rank, world;
    int (*allreduce_sum_f64)(void *user, void *buf_dev, int64_t count, void *stream);   /* in place, DEVICE pointer; 0 = ok */
    void *user;
} pk_comm;
int pk_svd_build_sharded(pk_ctx *ctx, pk_mat *A_local, const pk_comm *comm, int32_t k, int32_t block, double tol,
                         int32_t max_outer, uint64_t seed, double *sigma_out, double *V_out, double *U_out_local,
                         pk_build_stats *stats_out);
/* The k leading eigenpairs of a small dense symmetric PSD matrix T [n x n] (DEVICE, row-major, leading dimension ldt) — the
 * projected problem Q^T (A^T A) Q of the block Lanczos build (polara_amd/solver.py::_block_lanczos; inside the reference's
 * `svds` ARPACK solves the same kind of projected problem, models.py:844).  Filtered subspace iteration with locking on
 * the operator T, block width l (k <= l <= min(n, 1024)), run on `stream` (NULL: the context's) with temporaries from the
 * context's pool.  X0_dev: orthonormal start block [x0_rows x l] (rows x0_rows..n-1 are taken as zero: the warm start from
 * the pairs of a leading principal submatrix), or NULL = the first l unit vectors.  Convergence: ||T y - theta y|| <= tol *
 * theta_1 for the k leading pairs.  Outputs: basis_out_dev [n x l] (locked vectors, then the active block; column j belongs
 * to lam_out_host[j]), res_out_host[0 .. counts[1]) = residual norms of the active block, counts_out[5] = {locked vectors,
 * width of the active block, converged, outer iterations, products with T}.  Synchronises `stream` before it returns.
 * Round 6: the filter runs in SEGMENTS with a CholeskyQR between them and one Rayleigh-Ritz step per round (two host reads);
 * the iteration with locking takes over when that hands over (degenerate bounds, a Cholesky breakdown, stagnation).
 * lam0_host (or NULL): the Ritz values of the l columns of X0_dev when those are the pairs of a leading principal submatrix of
 * T (they keep their Rayleigh quotients), r0_rel: the worst relative residual of the first k of them w.r.t. THIS T (< 0:
 * unknown) — a warm look then needs no Rayleigh-Ritz step before its filter. */
int pk_sym_eig_topk_f64(pk_ctx *ctx, void *stream, int32_t n, const double *T_dev, int64_t ldt, int32_t k, int32_t l,
                        const double *X0_dev, int64_t ldx0, int32_t x0_rows, double tol, int32_t max_outer, uint64_t seed,
                        double *basis_out_dev, int64_t ldb, double *lam_out_host, double *res_out_host, int32_t *counts_out,
                        const double *lam0_host, double r0_rel);
/* What a host may choose about the builds of a context — explicit calls, not environment variables (round 6):
 *   "svd_method"   0 = the cost model (solver.py::choose_method restated), 1 = block Lanczos, 2 = filtered subspace iteration
 *   "krylov_block" 0 = the cost model (solver.py::choose_krylov_block restated), else the width of a Krylov block (<= block)
 *   "dist_overlap" two-panel exchange of a sharded product: 0 = never, 1 = by the cost model, 2 = whenever possible (tests)
 *   "hooi_ttm"     1 = pk_hooi runs the per-entry mode products (pk_ttm_f64) instead of the factored form
 *   "time_spmm"    1 = HIP events around every SpMM launch of the context's builds, read with pk_ctx_spmm_timings
 * Unknown names and values out of range are PK_E_INVALID. */
int pk_ctx_set_option(pk_ctx *ctx, const char *name, int32_t value);
/* The SpMM launches recorded since the last call (option "time_spmm"; bench.py's roofline of the build): waits for them,
 * writes min(count, cap) records — ms_out[i] = duration in ms, meta_out[6 i ..] = {rows written, rows gathered from, stored
 * entries, columns, bytes per stored value, bytes per element of the dense block} — forgets them all, returns the count. */
int64_t pk_ctx_spmm_timings(pk_ctx *ctx, double *ms_out, int64_t *meta_out, int64_t cap);
/* The recurrence of the block Lanczos build for a host layer that keeps the looks (polara_amd/solver.py::_block_lanczos; the
 * reference's `svds` call, models.py:841-844, runs ARPACK's recurrence in its place).  All three run on `stream` (a
 * hipStream_t; 0 = the null stream) with temporaries from the context's pool — use ONE stream per context.
 * pk_mat_wrap_device: a NON-OWNING matrix over CSR arrays that already live in HBM (indptr int64[n_rows + 1], indices int32,
 * values f32 | f64 — they must outlive the handle), with its task plan and the user-blocked transpose image sized for
 * products with `block_cols`-column blocks (0: 64).  pk_mat_free releases the handle, never the borrowed arrays.
 * pk_lanczos_steps: steps j0 + 1 .. j0 + m of the recurrence  W = A^T A Q_j;  T[:, j] = Q^T W;  Q_(j+1) R = W - Q T[:, j]
 * (shifted CholeskyQR3, re-projected against the whole basis in every pass) on the caller's buffers: Q_dev [n_cols x >=
 * (j0 + m + 1) b] with block j in columns [(j - 1) b, j b), T_dev [>= (j0 + m) b square] (block column j AND its mirror
 * image are written), S_out_dev [b x b] = W_perp^T W_perp of the LAST step run (the coupling behind the residual
 * estimates of the Ritz pairs), flags_dev[2] += Cholesky verdicts / max= distance of a last pass's Gram matrix from I.
 * last_closes: the last step of the call does not compute a next block (the space is full).  No host synchronisation.
 * rounded != 0: both sparse products of these steps gather fp32 images of their dense blocks (half the bytes per gathered
 * row, fp64 accumulation: a product rounded to ~6e-8 of its norm) and only the BAND of the block column of T is written —
 * for the late steps of a build only, when the pairs are within ~1e-7 of convergence (the error of a rounded product
 * enters a pair's residual times the pair's coefficients in that block; solver.py: products='relaxed').
 * pk_gramian_apply_f64: Z = A^T (A X), X / Z [n_cols x nc] with leading dimensions ldx / ldz (the verification product). */
int pk_mat_wrap_device(pk_ctx *ctx, void *stream, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *indptr_dev,
                       const int32_t *indices_dev, const void *values_dev, int32_t val_kind, int32_t block_cols,
                       pk_mat **mat_out);
int pk_lanczos_steps(pk_ctx *ctx, void *stream, pk_mat *A, int32_t b, int32_t j0, int32_t m, int32_t last_closes,
                     double *Q_dev, int64_t ldq, double *T_dev, int64_t ldt, double *S_out_dev, double *flags_dev,
                     int32_t rounded);
int pk_gramian_apply_f64(pk_ctx *ctx, void *stream, pk_mat *A, int32_t nc, const double *X_dev, int64_t ldx, double *Z_dev,
                         int64_t ldz);
/* The two halves of step j (j >= 1) for a host layer that shards the USERS itself — one process per GPU, item side replicated:
 * pk_lanczos_products writes W = A_p^T (A_p Q_j) of THIS rank's rows into W_out_dev [n_cols x b] (contiguous); the host sums W
 * over the ranks (ONE all-reduce of n_cols x b per step, e.g. ncclAllReduce on `stream`); pk_lanczos_orth then does on every
 * rank what pk_lanczos_steps does after its products: block column j of T and its mirror image, the next block by shifted
 * CholeskyQR3 re-projected in every pass, S_out_dev and flags_dev as there (`rounded`: band-only block column, see there). */
int pk_lanczos_products(pk_ctx *ctx, void *stream, pk_mat *A, int32_t b, int32_t j, const double *Q_dev, int64_t ldq,
                        double *W_out_dev, int32_t rounded);
int pk_lanczos_orth(pk_ctx *ctx, void *stream, int64_t n_items, int32_t b, int32_t j, int32_t last_closes, double *Q_dev, int64_t ldq,
                    double *T_dev, int64_t ldt, const double *W_dev, double *S_out_dev, double *flags_dev, int32_t rounded);
/* the context's HIP stream (hipStream_t as void*): what a pk_comm callback is handed, for hosts that create the
 * communicator's work on it */
void *pk_ctx_stream(pk_ctx *ctx);
/* Recommendations for the users of T (rows: test users, columns: the n_items items): scores = (T V) V^T, seen items
 * (every stored entry of T) pushed below all unseen ones when filter_seen, topk item ids per user by descending score
 * -> out_idx[n_users * topk] int64 row-major (the `top_recs` of models.py:400-405; -1 pads a user with fewer than topk
 * candidates when filter_seen = 0 is impossible: with filter_seen seen items re-enter after the unseen ones exactly as
 * models.py:510-519 orders them).  V_host: [n_items * K] column-major.  out_scores: fp64 scores of those items or NULL. */
int pk_score_topk(pk_ctx *ctx, int64_t n_items, int32_t K, const double *V_host, pk_mat *T, int32_t topk,
                  int32_t filter_seen, int64_t *out_idx, double *out_scores);
/* The same with the model-side state kept between calls — what a RecommenderModel keeps between get_recommendations()
 * calls (models.py:391-405: the factors and the test data do not change from call to call): pk_serving_create orders the
 * catalogue by factor norm, uploads the factors and their images, renames and re-sorts the rows of T and plans them;
 * pk_serving_score runs one scoring pass (any topk / filter_seen) and writes the caller's item ids; pk_score_topk =
 * create + score + free.  The handle belongs to `ctx`; T may be freed after pk_serving_create. */
typedef struct pk_serving pk_serving;
int pk_serving_create(pk_ctx *ctx, int64_t n_items, int32_t K, const double *V_host, pk_mat *T, pk_serving **out);
int pk_serving_score(pk_ctx *ctx, pk_serving *serving, int32_t topk, int32_t filter_seen, int64_t *out_idx,
                     double *out_scores);
void pk_serving_free(pk_ctx *ctx, pk_serving *serving);
/* Tucker / HOOI of a sparse 3-way tensor (`CoffeeModel.build` -> `hooi`, models.py:1009-1024, lib/tensor.py:37-96):
 * idx_host [nnz x 3] row-major (user, item, feedback level), vals_host or NULL (= ones, data.py:805), shape[3],
 * mlrank[3].  u1_start [n1 x r1] / u2_start [n2 x r2] (row-major, orthonormal columns): the start the reference draws
 * from NumPy's RandomState + LAPACK QR (tensor.py:57-63) — pass it to follow the reference's iteration exactly; both
 * NULL: a seeded device generator.  Outputs (host, row-major, C order like the reference's factors): u0 [n0 x r0],
 * u1 [n1 x r1], u2 [n2 x r2], core [r0 x r1 x r2], trace_out[num_iters] = the core norm after every iteration
 * (tensor.py:82-88), *iters_out = iterations run (stops when the core's growth falls below growth_tol). */
int pk_hooi(pk_ctx *ctx, int64_t nnz, const int64_t *idx_host, const double *vals_host, const int64_t *shape,
            const int32_t *mlrank, int32_t num_iters, double growth_tol, const double *u1_start, const double *u2_start,
            uint64_t seed, double *u0_out, double *u1_out, double *u2_out, double *core_out, double *trace_out,
            int32_t *iters_out);

#ifdef __cplusplus
}
#endif
#endif /* POLARA_HIP_H */
