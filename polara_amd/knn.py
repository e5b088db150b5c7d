"""Neighbourhood and random-walk item models: ItemKNN (cosine or Jaccard similarity with shrinkage, the K nearest neighbours
of every item) and P3alpha / RP3beta (C. Cooper et al., "Random walks in recommender systems", WWW 2014; B. Paudel et al.,
"Updatable, accurate, diverse, and scalable recommendations for interactive applications", TiiS 2016).  Both are "Gram
image, an element-wise normalisation, the K best of every row, a sparse W": the dense fp64 Gram image is the one EASE and
SLIM build (pk_i2i_build_f64 + pk_ease_diag_f64), the middle part is one fused pass (pk_knn_prune_f64, csrc/knn.hip: the
image is read once and n_items x K slots are written; the arithmetic is fixed in include/polara_hip.h, so the weights are
bit-equal to the NumPy restatement of tests/knn_reference.py applied to the same image), and the scores s_u = t_u W come
from the sparse x sparse scoring pass (pk_spsp_topk) SimilarityAggregation and SLIM run on; DESIGN.md 8s.

UserKNN has no image to start from (n_users^2 doubles): its neighbour pass forms every row of X X^T from the sparse operands
and prunes it in the same launch sequence (pk_spsp_knn_f64, csrc/uknn.hip: the sums of pk_spsp_topk, the arithmetic of
pk_knn_prune_f64), and its scores N_test X need a seen set that is not the left operand's own row (pk_spsp_topk_seen).  The
same pass builds ItemKNN and RP3beta without an image on request (`gram = 'sparse'`); DESIGN.md 8u.

Every scale vector (n_items or n_users numbers) is computed on the host in NumPy and uploaded.  The first part of this
module holds the setting checks and those vectors (pure Python and NumPy); the second part holds the models."""
from functools import partial
from timeit import default_timer as timer

import numpy as np

from . import i2i, simagg

# ---- planning ------------------------------------------------------------------------------------------------------
MAX_NEIGHBOURS = i2i.MAX_TOPK          # pk_knn_max_neighbours: the running list of a row is merged in 2 x 1024 keys of LDS
MAX_TOPK = simagg.MAX_TOPK             # the scoring pass is the sparse x sparse one
KINDS = {'scale': 0, 'cosine': 1, 'tanimoto': 2}      # PK_KNN_SCALE, PK_KNN_COSINE, PK_KNN_TANIMOTO
SIMILARITIES = ('cosine', 'jaccard')
GRAMS = ('image', 'sparse')            # the dense Gram image (default) or the sparse neighbour pass without one
DEFAULT_NEIGHBOURS = 100               # choices, not measurements
DEFAULT_BETA = 0.6


def check_similarity(value):
    if value not in SIMILARITIES:
        raise ValueError('similarity must be one of %s, got %r' % (', '.join(map(repr, SIMILARITIES)), value))
    return value


def check_gram(value):
    if value not in GRAMS:
        raise ValueError('gram must be one of %s, got %r' % (', '.join(map(repr, GRAMS)), value))
    return value


def check_neighbours(value):
    k = int(value)
    if k != value or not 1 <= k <= MAX_NEIGHBOURS:
        raise ValueError('neighbours must be an integer in 1..%d (pk_knn_max_neighbours), got %r' % (MAX_NEIGHBOURS, value))
    return k


def check_normalize(value):
    if not isinstance(value, (bool, np.bool_)) and value not in (0, 1):
        raise ValueError('normalize must be True or False, got %r' % (value,))
    return bool(value)


def _check_nonneg(name, value, upper=None):
    v = float(value)
    if not np.isfinite(v) or v < 0 or (upper is not None and v > upper):
        raise ValueError('%s must be a finite number %s, got %r' % (name, '>= 0' if upper is None else 'in [0, %g]' % upper, value))
    return v


check_shrink = partial(_check_nonneg, 'shrink')
check_asymmetric_alpha = partial(_check_nonneg, 'asymmetric_alpha', upper=1.0)
check_alpha = partial(_check_nonneg, 'alpha')
check_beta = partial(_check_nonneg, 'beta')


def power(v, exponent):
    """v ** exponent element-wise for a host fp64 vector v >= 0: np.sqrt for an exponent of exactly 0.5, np.power else."""
    v = np.asarray(v, dtype=np.float64)
    return np.sqrt(v) if exponent == 0.5 else np.power(v, float(exponent))


def inverse_power(v, exponent):
    """v ** -exponent where v > 0 and 0 elsewhere (np.power with the negated exponent)."""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(v.shape, dtype=np.float64)
    pos = v > 0
    out[pos] = np.power(v[pos], -float(exponent))
    return out


def cosine_vectors(q, asymmetric_alpha):
    """(row, col) of the pruning pass for the cosine: the TARGET is the row — row = q^(1 - alpha), col = q^alpha."""
    a = float(asymmetric_alpha)
    return power(q, 1.0 - a), power(q, a)


def squared_sums(keys, vals, n):
    """sum of vals^2 per key (np.bincount over the given order): the squared norms q of the rows or the columns of a CSR."""
    vals = np.asarray(vals, dtype=np.float64)
    return np.bincount(keys, weights=vals * vals, minlength=n)


def rp3_vectors(d_user, d_item, pop, alpha, beta):
    """(user scale d_u^(-alpha / 2), row d_i^(-alpha), col pop^(-beta)), each 0 where its count is 0."""
    return inverse_power(d_user, float(alpha) / 2.0), inverse_power(d_item, alpha), inverse_power(pop, beta)


# ---- models ----------------------------------------------------------------------------------------------------------
from .models import _ItemWeightModel, _setting     # noqa: E402  (the planning part above needs neither)


class _NeighbourModel(_ItemWeightModel):
    """What every model of this module shares: `neighbours` and `normalize`, dense output by default, scores through the
    sparse x sparse pass, feedback >= 0."""
    _topk_limit = simagg.MAX_TOPK

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._neighbours = DEFAULT_NEIGHBOURS
        self._normalize = False
        self._dense_output = True

    neighbours = _setting('neighbours', '_renew_model', 'entries kept per row (1..1024): a change renews the model',
                          check=check_neighbours)
    normalize = _setting('normalize', '_renew_model', "the kept weights divided by their absolute sum: a change renews the model",
                         check=check_normalize)

    def _nonnegative_training_csr(self):
        A = self._training_device_csr()
        bad = int((A.values < 0).sum().item()) if A.nnz else 0
        if bad:
            raise ValueError('%s: %d of %d feedback values are negative (the similarities and the walk need feedback >= 0)'
                             % (self.method, bad, A.nnz))
        return A

    def _host_triplet(self, A):
        """(row of every stored entry, its column, its fp64 value) of a device CSR, in its stored order."""
        ops = self.ops
        indptr, cols, vals = ops.to_host(A.indptr), ops.to_host(A.indices), ops.csr_values_host(A)
        return np.repeat(np.arange(A.shape[0]), np.diff(indptr)), cols, vals


class _PrunedItemModel(_NeighbourModel):
    """What ItemKNNModel and RP3BetaModel share: `item_weights`, the canonical device CSR of W [n_items x n_items]
    (W[i, j]: the weight of source item i for target item j; sorted indices, no stored zeros, no diagonal), scored through
    the sparse x sparse pass; `gram`; the build's frame (memory guard, stages, statistics)."""
    _weight_slots = ('_W',)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._gram = 'image'

    gram = _setting('gram', '_renew_model', "'image' (default): the dense Gram image is built and pruned; 'sparse': the rows "
                    "of the Gram matrix are formed from the sparse operands and pruned without an image, for catalogues whose "
                    "image does not fit.  Never switched automatically: a change renews the model", check=check_gram)

    @property
    def item_weights(self):
        """The canonical device CSR of W [n_items x n_items] (None before the build)."""
        return self._W

    def _operand(self):
        return self._W

    def build(self):
        self._single_process()
        ops = self.ops
        self._release_weights()
        A = self._nonnegative_training_csr()
        n_items = int(A.shape[1])
        image = self.gram == 'image'
        if image:
            i2i.check_build_memory(n_items, ops.free_bytes())       # speaks before the image or anything of the build exists
        stages = {'gram_s': 0.0, 'prune_s': 0.0, 'transpose_s': 0.0}
        start = timer()
        W = (self._weights if image else self._weights_sparse)(A, n_items, partial(self._stage, stages))
        self._track(start)
        self._W = W
        self.build_stats = dict(stages, n_items=n_items, nnz=int(W.nnz), image_bytes=i2i.build_image_bytes(n_items) if image else 0,
                                neighbours=self.neighbours, training_nnz=int(A.nnz), gram=self.gram)


def _similarity_vectors(similarity, q_rows, q_cols, asymmetric_alpha):
    """(kind, row, col) of the neighbour pass for squared norms q_rows of its rows and q_cols of its columns."""
    if similarity == 'cosine':
        return KINDS['cosine'], cosine_vectors(q_rows, asymmetric_alpha)[0], cosine_vectors(q_cols, asymmetric_alpha)[1]
    return KINDS['tanimoto'], q_rows, q_cols


class ItemKNNModel(_PrunedItemModel):
    """ItemKNN.  With q the diagonal of G = X^T X (X under the implicit rule when `implicit`):
    `similarity` 'cosine' (default): W[i, j] = g_ij / (q_i^alpha q_j^(1 - alpha) + shrink), alpha = `asymmetric_alpha`
    (0.5: the plain cosine); 'jaccard' (Tanimoto on real values): W[i, j] = g_ij / ((q_i + q_j - g_ij) + shrink).  Every
    TARGET item j keeps its `neighbours` (100) best sources, ties to the lower item; `normalize` divides a target's kept
    weights by their absolute sum.  `shrink` (0.0) >= 0.  A change of any of these renews the model; `dense_output` and the
    candidate rules are SLIMModel's.  Single process; INTEGRATION.md has the semantics."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'ItemKNN'
        self._similarity = 'cosine'
        self._shrink = 0.0
        self._asymmetric_alpha = 0.5

    similarity = _setting('similarity', '_renew_model', "'cosine' or 'jaccard': a change renews the model", check=check_similarity)
    shrink = _setting('shrink', '_renew_model', 'added to every denominator (>= 0): a change renews the model', check=check_shrink)
    asymmetric_alpha = _setting('asymmetric_alpha', '_renew_model', 'the exponent of the source norm of the cosine (in [0, 1]): '
                                'a change renews the model', check=check_asymmetric_alpha)

    def _weights(self, A, n_items, stage):
        """Gram image with its diagonal -> the rows pruned with the TARGET as the row -> device transpose."""
        ops = self.ops
        G = stage('gram', lambda: ops.knn_gram(A))
        q = ops.to_host(G.diagonal()[:n_items])                      # n_items numbers
        if self.similarity == 'cosine':
            kind, (row, col) = KINDS['cosine'], cosine_vectors(q, self.asymmetric_alpha)
        else:
            kind, row, col = KINDS['tanimoto'], q, q
        Wt = stage('prune', lambda: ops.knn_prune(G, n_items, kind, row, col, self.shrink, self.neighbours, self.normalize))
        del G
        return stage('transpose', lambda: ops.csr_transpose(Wt))     # the rows of W^T are not kept

    def _weights_sparse(self, A, n_items, stage):
        """The TARGET rows of X^T X formed from X^T and X and pruned in one pass (pk_spsp_knn_f64; 'gram' holds the
        transpose of X and q, the squared column norms summed in X's stored order) -> device transpose."""
        ops = self.ops

        def operands():
            _, cols, vals = self._host_triplet(A)
            return ops.csr_transpose(A), squared_sums(cols, vals, n_items)
        At, q = stage('gram', operands)
        kind, row, col = _similarity_vectors(self.similarity, q, q, self.asymmetric_alpha)
        exclude = np.arange(n_items, dtype=np.int32)
        Wt = stage('prune', lambda: ops.spsp_knn(At, A, kind, row, col, self.shrink, self.neighbours, self.normalize, exclude))
        return stage('transpose', lambda: ops.csr_transpose(Wt))


class RP3BetaModel(_PrunedItemModel):
    """RP3beta: W[i, j] = pop_j^(-beta) sum_u (a_ui / d_i)^alpha (a_uj / d_u)^alpha with d_u the row sums and d_i the column
    sums of the training matrix and pop_j the number of stored positive entries of item j — the three-step walk item ->
    user -> item with the transition probabilities raised to `alpha` (1.0) and the popularity of the target discounted by
    `beta` (0.6).  Built as r_i G'[i, j] c_j with G' the Gram image of X' = diag(d_u^(-alpha / 2)) A^alpha (element-wise
    power), r = d_i^(-alpha), c = pop^(-beta).  Every SOURCE item i keeps its `neighbours` (100) best targets, ties to the
    lower item; `normalize` divides a source's kept weights by their sum.  Feedback must be >= 0.  A change of a setting
    renews the model; `dense_output` and the candidate rules are SLIMModel's.  Single process."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'RP3beta'
        self._alpha = 1.0
        self._beta = DEFAULT_BETA

    alpha = _setting('alpha', '_renew_model', 'the exponent of the transition probabilities (>= 0): a change renews the model',
                     check=check_alpha)
    beta = _setting('beta', '_renew_model', "the exponent of the target's popularity (>= 0): a change renews the model",
                    check=check_beta)

    def _transformed(self, A):
        """(X', r, c): the device CSR X' = diag(d_u^(-alpha / 2)) A^alpha (fp64) and the host vectors of the pruning pass."""
        ops = self.ops
        n_users, n_items = A.shape
        rows, cols, vals = self._host_triplet(A)
        d_user = np.bincount(rows, weights=vals, minlength=n_users)
        d_item = np.bincount(cols, weights=vals, minlength=n_items)
        pop = np.bincount(cols[vals > 0], minlength=n_items).astype(np.float64)
        su, r, c = rp3_vectors(d_user, d_item, pop, self.alpha, self.beta)
        return ops.csr_row_scaled_power(A, su, self.alpha), r, c

    def _weights(self, A, n_items, stage):
        """X' -> its Gram image -> the rows scaled and pruned directly (a source keeps its best targets): no transpose."""
        ops = self.ops
        X, r, c = stage('gram', lambda: self._transformed(A))
        G = stage('gram', lambda: ops.knn_gram(X))
        return stage('prune', lambda: ops.knn_prune(G, n_items, KINDS['scale'], r, c, 0.0, self.neighbours, self.normalize))

    def _weights_sparse(self, A, n_items, stage):
        """X' -> the rows of X'^T X' formed from the sparse operands, scaled and pruned directly (pk_spsp_knn_f64); an item
        is excluded from its own row, as the image pass excludes the diagonal."""
        ops = self.ops
        X, r, c = stage('gram', lambda: self._transformed(A))
        Xt = stage('gram', lambda: ops.csr_transpose(X))
        exclude = np.arange(n_items, dtype=np.int32)
        return stage('prune', lambda: ops.spsp_knn(Xt, X, KINDS['scale'], r, c, 0.0, self.neighbours, self.normalize, exclude))


class P3AlphaModel(RP3BetaModel):
    """P3alpha: RP3beta without the popularity discount (`beta` fixed at 0)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'P3alpha'
        self._beta = 0.0

    @property
    def beta(self):
        return 0.0

    @beta.setter
    def beta(self, value):
        if check_beta(value) != 0.0:
            raise ValueError('P3alpha: beta is fixed at 0 (RP3BetaModel has the popularity discount)')


class UserKNNModel(_NeighbourModel):
    """UserKNN.  With X the training matrix (under the implicit rule when `implicit`), g_uv = sum_i x_ui x_vi and
    q_v = sum_i x_vi^2: `similarity` 'cosine' (default): N[u, v] = g_uv / (q_u^(1 - alpha) q_v^alpha + shrink), alpha =
    `asymmetric_alpha` (0.5: the plain cosine; the TARGET user u is the row); 'jaccard' (Tanimoto on real values):
    N[u, v] = g_uv / ((q_u + q_v - g_uv) + shrink).  Every target user keeps its `neighbours` (100) best training users, ties
    to the lower user, never itself; `normalize` divides a user's kept weights by their absolute sum.  Scores are
    s_u = sum_v N[u, v] x_v.  A known test user takes its row of `user_weights`; under warm start the neighbours of the test
    rows are computed by the same kernel from their interactions (no user is excluded).  No n_users x n_users image exists
    at any point: rows of X X^T are formed from the sparse operands and pruned in one pass (pk_spsp_knn_f64).  A change of
    a setting renews the model; `dense_output` and the candidate rules are SLIMModel's.  Feedback must be >= 0.  Single
    process; INTEGRATION.md has the semantics."""
    _weight_slots = ('_N', '_X', '_Xt', '_q')
    _operand_noun = 'training matrix'

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'UserKNN'
        self._slice_users = None               # the data-level users of the slice being scored (slice_recommendations)
        self._similarity = 'cosine'
        self._shrink = 0.0
        self._asymmetric_alpha = 0.5

    similarity = ItemKNNModel.similarity
    shrink = ItemKNNModel.shrink
    asymmetric_alpha = _setting('asymmetric_alpha', '_renew_model', 'the exponent of the neighbour norm of the cosine (in [0, 1]): '
                                'a change renews the model', check=check_asymmetric_alpha)

    @property
    def user_weights(self):
        """The canonical device CSR of N [n_users x n_users] over the training users (None before the build)."""
        return self._N

    def _operand(self):
        return self._X

    def _neighbours_of(self, L, exclude):
        """The pruned rows of L X^T as a canonical device CSR [rows of L x n_users]; row norms from L's own values."""
        rows, _, vals = self._host_triplet(L)
        kind, row, col = _similarity_vectors(self.similarity, squared_sums(rows, vals, L.shape[0]), self._q, self.asymmetric_alpha)
        return self.ops.spsp_knn(L, self._Xt, kind, row, col, self.shrink, self.neighbours, self.normalize, exclude)

    def build(self):
        self._single_process()
        ops = self.ops
        self._release_weights()
        X = self._nonnegative_training_csr()
        n_users = int(X.shape[0])
        stages = {'upload_s': 0.0, 'neighbours_s': 0.0}
        start = timer()

        def operands():
            rows, _, vals = self._host_triplet(X)
            return ops.csr_transpose(X), squared_sums(rows, vals, n_users)
        self._X = X
        self._Xt, self._q = self._stage(stages, 'upload', operands)
        N = self._stage(stages, 'neighbours', lambda: self._neighbours_of(X, np.arange(n_users, dtype=np.int32)))
        self._track(start)
        self._N = N
        self.build_stats = dict(stages, n_users=n_users, nnz=int(N.nnz), neighbours=self.neighbours, training_nnz=int(X.nnz))

    # ---- scoring: s = N_test X with the test rows' own entries as the seen set ----------------------------------------
    def _test_neighbours(self, T, users):
        """N_test [rows of T x n_users]: warm start — the neighbours of the rows of T (under the implicit rule); else the
        rows `users` (data-level ids; None: those of the test data) of `user_weights`."""
        if self.data.warm_start:
            return self._neighbours_of(T, None)
        ids = np.asarray(self._get_test_data()[2] if users is None else users, dtype=np.int64)
        N, n_users = self._N, self._N.shape[0]
        if len(ids) != T.shape[0] or (len(ids) and (ids.min() < 0 or ids.max() >= n_users)):
            raise ValueError('%s: %d test rows for %d user ids within %d training users' % (self.method, T.shape[0], len(ids), n_users))
        if len(ids) == n_users and np.array_equal(ids, np.arange(n_users)):
            return N
        return self.ops.csr_gather_rows(N, ids)

    def _score(self, T, n_items, want_scores=False, users=None):
        ops, X = self.ops, self._X
        if n_items != X.shape[1]:
            raise ValueError('test data over %d items, the %s over %d' % (n_items, self._operand_noun, X.shape[1]))
        T = self._test_values(T)
        recs, scores = ops.spsp_topk_seen(self._test_neighbours(T, users), X, T, self.topk, self.filter_seen,
                                          sparse=not self.dense_output, want_scores=want_scores)
        return (recs, scores) if want_scores else recs

    def slice_recommendations(self, test_data, shape, start, stop, test_users=None):
        stop = min(stop, shape[0])
        if not self.data.warm_start:
            users = self._get_test_data()[2] if test_users is None else test_users
            self._slice_users = np.asarray(users)[start:stop]
        try:
            return super().slice_recommendations(test_data, shape, start, stop, test_users)
        finally:
            self._slice_users = None

    def _slice_scores(self, T, n_items):
        ops = self.ops
        return ops.to_host(ops.spsp_rows(self._test_neighbours(T, self._slice_users), self._X))
