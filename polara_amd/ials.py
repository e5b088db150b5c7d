"""Implicit ALS — iALS / WRMF (polara/recommender/external/implicit/ialswrapper.py): the factorisation of Hu, Koren and
Volinsky, "Collaborative filtering for implicit feedback datasets" (2008).  The reference hands the work to the third-party
`implicit` package; here the solver is the library's own (csrc/ials.hip): an alternating sequence of half-steps, each solving
for every row of the sparse confidence matrix a k x k normal-equations system EXACTLY (Cholesky, fp64) — no conjugate-gradient
approximation, no float32.  The same kernel folds in warm-start users against the built item factors.

The objective, with c the confidences on the stored entries:
    sum over ALL (u, i) of w_ui (p_ui - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2),   w = c, p = 1 stored;  w = 1, p = 0 elsewhere.
A half-step minimises it exactly over one factor matrix, so it never increases.

Initial factors are this package's own convention (`initial_factors`); no equality with any build of the `implicit` package is
claimed.  Single process."""
from timeit import default_timer as timer

import numpy as np

from .factor_serving import FactorQueriesMixin
from .models import RecommenderModel


def initial_factors(n_users, n_items, rank, seed=None):
    """(X0, Y0): uniform [0, 0.01) draws, X first, then Y, from `RandomState(seed)` or NumPy's global generator.  X0 is
    overwritten by the first half-step; it is drawn so that the position of the stream is defined."""
    rnds = np.random if seed is None else np.random.RandomState(seed)
    X0 = rnds.rand(int(n_users), int(rank)) * 0.01
    Y0 = rnds.rand(int(n_items), int(rank)) * 0.01
    return X0, Y0


def ials_fit(ops, C, rank, regularization, num_epochs, seed=None, init=None, loss_history=None, iter_time=None, comm=None):
    """`num_epochs` times (user half-step, item half-step) on the ops-level CSR of confidences C [n_users x n_items].
    Returns the DEVICE blocks (X, Y).  loss_history: a list that receives the objective after EVERY half-step (two entries
    per epoch); init = (X0, Y0) host arrays instead of the seeded draw."""
    if comm is not None and getattr(comm, 'world', 1) > 1:
        raise NotImplementedError('iALS: multi-process builds are not supported (comm.world = %d)' % comm.world)
    n_users, n_items = (int(x) for x in C.shape)
    rank = int(rank)
    if rank < 1 or rank > ops.ials_max_rank():
        raise ValueError('iALS: rank %d outside 1..%d' % (rank, ops.ials_max_rank()))
    Ct = C.T                                                    # one transpose (pk_csr_transpose), kept on the matrix
    if init is None:
        init = initial_factors(n_users, n_items, rank, seed)
    X0, Y0 = (np.asarray(a, dtype=np.float64) for a in init)
    if X0.shape != (n_users, rank) or Y0.shape != (n_items, rank):
        raise ValueError('iALS: initial factors of shapes %s, %s for (%d x %d), (%d x %d)'
                         % (X0.shape, Y0.shape, n_users, rank, n_items, rank))
    X, Y = ops.to_device(np.ascontiguousarray(X0)), ops.to_device(np.ascontiguousarray(Y0))
    lam = float(regularization)
    GY = ops.gram(Y)
    for _ in range(int(num_epochs)):
        start = timer()
        ops.ials_half_step(C, Y, lam, out=X, G=GY)
        GX = ops.gram(X)
        if loss_history is not None:
            loss_history.append(ops.ials_loss(C, X, Y, lam, GX=GX, GY=GY))
        ops.ials_half_step(Ct, X, lam, out=Y, G=GX)
        GY = ops.gram(Y)
        if loss_history is not None:
            loss_history.append(ops.ials_loss(C, X, Y, lam, GX=GX, GY=GY))
        if iter_time is not None:
            iter_time.append(timer() - start)
    return X, Y


class ImplicitALS(FactorQueriesMixin, RecommenderModel):
    """ialswrapper.py:13-91.  `factors` holds host fp64 arrays — users [n_users x k], items [n_items x k]; `loss_history`
    (with `compute_loss`) the objective after every half-step; `num_threads` is accepted and ignored.  Warm start folds the
    test users in by one user half-step against the built item factors (the library's `recalculate_user=True`).  A rank
    change invalidates the model."""

    def __init__(self, *args, seed=None, compute_loss=False, **kwargs):
        self.seed = seed
        self.compute_loss = compute_loss
        super().__init__(*args, **kwargs)
        self._rank = 10
        self.alpha = 1
        self.epsilon = 1
        self.weight_func = np.log2
        self.regularization = 0.01
        self.num_threads = 0
        self.num_epochs = 15
        self.method = 'iALS'
        self.factors = {}
        self.loss_history = None
        self.iterations_time = None
        self._factors_dev = None            # (host user factors of `factors`, X on the device) of the last build
        self._items_dev = None              # (host item factors of `factors`, Y on the device in the data's item order, Y^T Y)
        self.data.subscribe(self.data.on_change_event, self._clean_metadata)

    def _clean_metadata(self):
        super()._clean_metadata()
        self._items_dev = None

    @staticmethod
    def confidence(values, alpha=1, weight=None, epsilon=1, dtype='double'):
        """the wrapper's generic confidence: alpha * weight(values / epsilon), or alpha * values / epsilon without a weight"""
        scaled = values / epsilon
        if weight is not None:
            scaled = weight(scaled)
        return (alpha * scaled).astype(dtype)

    def _confidence_csr(self, A):
        """`A` with `confidence` applied to its stored values — on the host: `weight_func` is any callable and the result is
        the wrapper's arithmetic (one download and one upload of nnz doubles).  Entries of confidence exactly 0 are dropped
        (with the default log2 a feedback of 1 is "unobserved"); a negative or non-finite confidence raises."""
        ops = self.ops
        with np.errstate(divide='ignore', invalid='ignore'):
            conf = np.asarray(self.confidence(ops.csr_values_host(A), alpha=self.alpha, weight=self.weight_func, epsilon=self.epsilon),
                              dtype=np.float64)
        bad = int((~np.isfinite(conf) | (conf < 0)).sum())
        if bad:
            raise ValueError('%s: %d of %d confidence values are negative or not finite (alpha * weight_func(feedback / epsilon) '
                             'must be >= 0; negative preferences are not supported)' % (self.method, bad, len(conf)))
        return ops.csr_replace_values(A, conf, drop_zeros=True)

    def build(self):
        self._require_single_process_build()
        ops = self.ops
        rank = int(self.rank)
        if rank < 1 or rank > ops.ials_max_rank():
            raise ValueError('%s: rank %d outside 1..%d' % (self.method, rank, ops.ials_max_rank()))
        C = self._confidence_csr(self._training_device_csr())      # scaling (ScaledMatrixMixin) first, confidence second
        self.loss_history = [] if self.compute_loss else None
        self.iterations_time = []
        start = timer()
        X, Y = ials_fit(ops, C, rank, self.regularization, self.num_epochs, seed=self.seed, loss_history=self.loss_history,
                        iter_time=self.iterations_time)
        ops.synchronize()
        self._track(start)
        self._set_factors(X, Y)
        self._items_dev = (self.factors[self.data.fields.itemid], Y, None)

    # ---- warm start: the fold-in ----------------------------------------------------------------------------------------
    def _item_factors_block(self):
        """(Y [n_items x k] on the device in the DATA's item order — the column order of the fold-in matrix —, Y^T Y)"""
        Y = self.factors.get(self.data.fields.itemid, None)
        if Y is None:
            raise ValueError('%s: no item factors (build the model first)' % self.method)
        kept = self._items_dev
        if kept is None or kept[0] is not Y:
            kept = (Y, self.ops.to_device(np.ascontiguousarray(Y, dtype=np.float64)), None)
        if kept[2] is None:
            kept = (kept[0], kept[1], self.ops.gram(kept[1]))
        self._items_dev = kept
        return kept[1], kept[2]

    def fold_in_matrix(self):
        """The confidences of the test users' known feedback as an ops-level CSR [n_test_users x n_items] in the data's item
        order: feedback of exactly 0 never enters (models.py:180-211), then `confidence`, then entries of confidence 0 are
        dropped.  (Both kinds of entries stay "seen": the scoring pass masks them through the test matrix of the pass.)"""
        test_data, shape, _ = self._get_test_data()
        users, items, feedback = (np.asarray(a) for a in test_data)
        keep = np.flatnonzero(feedback)
        T = self.ops.csr_from_coo(np.ascontiguousarray(users[keep], dtype=np.int64), np.ascontiguousarray(items[keep], dtype=np.int64),
                                  np.asarray(feedback[keep], dtype=np.float64), (int(shape[0]), int(shape[1])))
        return self._confidence_csr(T)

    def fold_in(self):
        """the warm-start users' factors [n_test_users x k] on the device (a view with an even leading dimension): one user
        half-step on `fold_in_matrix` against the built item factors"""
        ops = self.ops
        Y, GY = self._item_factors_block()
        Cw = self.fold_in_matrix()
        k = int(Y.shape[1])
        block = ops.zeros(int(Cw.shape[0]), k + (k & 1))
        ops.ials_half_step(Cw, Y, float(self.regularization), out=block[:, :k], G=GY)
        return block[:, :k]

    def _check_serving(self):
        if self.data.warm_start and self.filter_seen is False:
            raise ValueError('The model always filters seen items from results.')

    def _test_queries(self, test_users, start=0, stop=None):
        if self.data.warm_start:
            return self.fold_in()[start:stop]
        return super()._test_queries(test_users, start, stop)
