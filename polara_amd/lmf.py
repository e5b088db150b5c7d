"""Logistic matrix factorisation — LMF (polara/recommender/external/implicit: the third factor model of the third-party
`implicit` package next to ALS and BPR): Johnson, "Logistic matrix factorization for implicit feedback data" (2014), in the shape
that package trains it — rank k plus a bias on either side, alternating full-batch AdaGrad steps, sampled negatives.  Here the
solver is the library's own (csrc/lmf.hip).

Factors carry K = k + 2 columns: the user block X = [factors | bias | 1], the item block Y = [factors | 1 | bias], so that
X @ Y.T are the logits — and the scores served.  With c the confidences on the stored entries the model ascends
    sum over stored (u, i) of c_ui log sigma(s_ui)  +  sum over SAMPLED (u, i) of log sigma(-s_ui)  -  lambda / 2 (|X|^2 + |Y|^2)
in alternating half-steps: a user half-step moves every row of X against the fixed Y by ONE AdaGrad step on the gradient
    sum over the row's entries of c sigma(-s) y_i  -  sum over SAMPLED i of sigma(s) y_i  -  lambda x_u,
then an item half-step does the same for Y on the transposed confidences against the new X.  The second sum is `implicit`'s
estimate of the sum over all items: min(n_other, n * neg_prop) columns drawn uniformly over ALL columns, with replacement — the
row's own entries are NOT excluded (a drawn positive enters once more, as a negative; that is the convention of `implicit`, whose
sampled term stands for the sum over every item, liked ones included).  The draws come from a counter inside the kernel: no
sample array exists.  The constant-1 columns are never touched; the AdaGrad state starts at zero and is kept over the epochs.

Against `implicit`: fp64, not float32; the order of every sum is fixed, so runs are bit-reproducible; the draw stream and the
initial factors are this package's own (`initial_factors`) — no equality with any build of `implicit` is claimed.  The arithmetic
of a half-step is spelled out in include/polara_hip.h and derived in DESIGN.md.  Single process."""
from timeit import default_timer as timer

import numpy as np

from .factor_serving import FactorQueriesMixin
from .ials import ImplicitALS
from .models import RecommenderModel

FOLD_IN_ROUND = 0x80000000          # the rounds of a fold-in: this bit set, so that its stream never meets a build's


def initial_factors(n_users, n_items, rank, seed=None):
    """(X0 [n_users x (k + 2)], Y0 [n_items x (k + 2)]): `normal(scale=0.1)` draws for the k factor columns, X first, then Y,
    from `RandomState(seed)` or NumPy's global generator; the biases (column k of X0, k + 1 of Y0) are 0 and the pinned columns
    (k + 1 of X0, k of Y0) are 1.  This package's own convention: no equality with any build of `implicit` is claimed."""
    rnds = np.random if seed is None else np.random.RandomState(seed)
    k = int(rank)
    X0, Y0 = np.zeros((int(n_users), k + 2)), np.zeros((int(n_items), k + 2))
    X0[:, :k] = rnds.normal(scale=0.1, size=(int(n_users), k))
    Y0[:, :k] = rnds.normal(scale=0.1, size=(int(n_items), k))
    X0[:, k + 1] = 1.0
    Y0[:, k] = 1.0
    return X0, Y0


def lmf_fit(ops, C, rank, learning_rate, regularization, neg_prop, num_epochs, seed=None, init=None, iter_time=None, stats=None,
            comm=None):
    """`num_epochs` times (user half-step, item half-step) on the ops-level CSR of confidences C [n_users x n_items]; half-step
    `side` of epoch `e` draws its negatives from the stream (seed, round = 2 e + side).  Returns the DEVICE blocks (X, Y) of
    k + 2 columns.  seed: 32 unsigned bits (None: one draw from NumPy's global generator, reported in `stats`); it seeds the
    initial factors and the negatives.  init = (X0, Y0) host arrays of k + 2 columns instead of the seeded draw.  stats
    receives the seed, the epochs and the negatives per half-step."""
    if comm is not None and getattr(comm, 'world', 1) > 1:
        raise NotImplementedError('LMF: multi-process builds are not supported (comm.world = %d)' % comm.world)
    n_users, n_items = (int(x) for x in C.shape)
    rank, neg_prop = int(rank), int(neg_prop)
    if rank < 1 or rank > ops.lmf_max_rank():
        raise ValueError('LMF: rank %d outside 1..%d' % (rank, ops.lmf_max_rank()))
    if neg_prop < 1:
        raise ValueError('LMF: neg_prop %d < 1' % neg_prop)
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 32, dtype=np.uint64))
    seed = int(seed)
    if not 0 <= seed < 2 ** 32:
        raise ValueError('LMF: the seed %d does not fit 32 unsigned bits' % seed)
    K = rank + 2
    X0, Y0 = (np.asarray(a, dtype=np.float64) for a in (initial_factors(n_users, n_items, rank, seed) if init is None else init))
    if X0.shape != (n_users, K) or Y0.shape != (n_items, K):
        raise ValueError('LMF: initial factors of shapes %s, %s for (%d x %d), (%d x %d)' % (X0.shape, Y0.shape, n_users, K, n_items, K))
    users, items = ops.lmf_plan(C, neg_prop), ops.lmf_plan(C.T, neg_prop)    # one transpose and two plans, kept on the matrix
    X, Y = ops.to_device(np.ascontiguousarray(X0)), ops.to_device(np.ascontiguousarray(Y0))
    AX, AY = ops.zeros(n_users, K), ops.zeros(n_items, K)
    for epoch in range(int(num_epochs)):
        start = timer()
        ops.lmf_half_step(users, Y, X, AX, learning_rate, regularization, seed, 2 * epoch, K - 1)
        ops.lmf_half_step(items, X, Y, AY, learning_rate, regularization, seed, 2 * epoch + 1, K - 2)
        if iter_time is not None:
            iter_time.append(timer() - start)
    if stats is not None:
        stats.update(seed=seed, epochs=int(num_epochs), neg_prop=neg_prop, user_negatives=users['negatives'],
                     item_negatives=items['negatives'])
    return X, Y


class ImplicitLMF(FactorQueriesMixin, RecommenderModel):
    """`implicit`'s LogisticMatrixFactorization behind the interface of the reference's `implicit` wrappers, with that package's
    defaults: rank 30, learning_rate 1.0, regularization 0.6, neg_prop 30, num_epochs 30.  The confidences are ImplicitALS's:
    alpha * weight_func(feedback / epsilon), entries of confidence 0 dropped, negative or non-finite ones refused.  `factors`
    holds host fp64 arrays of k + 2 columns — users [factors | bias | 1], items [factors | 1 | bias] —, so that their product
    is the scores; `build_stats` the seed, the epochs and the negatives per half-step.  `random_state` (or `seed=`) seeds the
    build; `num_threads` and `show_progress` are accepted and ignored.  Negatives are uniform over ALL items, the user's own
    included (the module's docstring).  Warm start folds the test users in by `fold_in_epochs` user half-steps of the same
    kernel against the built item factors, from zero factors and zero AdaGrad state.  A rank change invalidates the model."""

    def __init__(self, *args, seed=None, **kwargs):
        self.random_state = seed
        super().__init__(*args, **kwargs)
        self._rank = 30
        self.alpha = 1
        self.epsilon = 1
        self.weight_func = np.log2
        self.learning_rate = 1.0
        self.regularization = 0.6
        self.neg_prop = 30
        self.num_epochs = 30
        self.fold_in_epochs = 10
        self.num_threads = 0
        self.show_progress = False
        self.method = 'LMF'
        self.factors = {}
        self.iterations_time = None
        self.build_stats = {}
        self._factors_dev = None            # (host user factors of `factors`, X on the device) of the last build
        self._items_dev = None              # (host item factors of `factors`, Y on the device in the data's item order)
        self.data.subscribe(self.data.on_change_event, self._clean_metadata)

    @property
    def seed(self):
        return self.random_state

    @seed.setter
    def seed(self, value):
        self.random_state = value

    def _clean_metadata(self):
        super()._clean_metadata()
        self._items_dev = None

    # the confidence transform and the fold-in matrix are iALS's own: one copy, under this model's name in its messages
    confidence = staticmethod(ImplicitALS.confidence)
    _confidence_csr = ImplicitALS._confidence_csr
    fold_in_matrix = ImplicitALS.fold_in_matrix

    def _check_hyperparameters(self):
        ops = self.ops
        rank, neg_prop = int(self.rank), int(self.neg_prop)
        if rank < 1 or rank > ops.lmf_max_rank():
            raise ValueError('%s: rank %d outside 1..%d' % (self.method, rank, ops.lmf_max_rank()))
        if neg_prop < 1:
            raise ValueError('%s: neg_prop %d < 1' % (self.method, neg_prop))
        return rank, neg_prop

    def build(self):
        self._require_single_process_build()
        ops = self.ops
        rank, neg_prop = self._check_hyperparameters()
        C = self._confidence_csr(self._training_device_csr())      # scaling (ScaledMatrixMixin) first, confidence second
        self.iterations_time = []
        stats = {}
        start = timer()
        X, Y = lmf_fit(ops, C, rank, self.learning_rate, self.regularization, neg_prop, self.num_epochs, seed=self.random_state,
                       iter_time=self.iterations_time, stats=stats)
        ops.synchronize()
        self._track(start)
        self.build_stats = stats
        self._set_factors(X, Y)
        self._items_dev = (self.factors[self.data.fields.itemid], Y)

    # ---- warm start: the fold-in ----------------------------------------------------------------------------------------
    def _item_factors_block(self):
        """Y [n_items x (k + 2)] on the device in the DATA's item order — the column order of the fold-in matrix"""
        Y = self.factors.get(self.data.fields.itemid, None)
        if Y is None:
            raise ValueError('%s: no item factors (build the model first)' % self.method)
        kept = self._items_dev
        if kept is None or kept[0] is not Y:
            kept = self._items_dev = (Y, self.ops.to_device(np.ascontiguousarray(Y, dtype=np.float64)))
        return kept[1]

    def fold_in(self):
        """the warm-start users' rows [n_test_users x (k + 2)] on the device: `fold_in_epochs` user half-steps on
        `fold_in_matrix` against the built item factors, from factors 0, bias 0, the pinned 1 and AdaGrad state 0; half-step t
        draws from the stream (the build's seed, round 0x80000000 | t).  A user without a confidence to fold in keeps that start."""
        ops = self.ops
        _, neg_prop = self._check_hyperparameters()
        Y = self._item_factors_block()
        Cw = self.fold_in_matrix()
        K = int(Y.shape[1])
        block = ops.zeros(int(Cw.shape[0]), K + (K & 1))
        X, A = block[:, :K], ops.zeros(int(Cw.shape[0]), K)
        X[:, K - 1] = 1.0
        plan = ops.lmf_plan(Cw, neg_prop)
        seed = self.build_stats.get('seed', self.random_state)
        for t in range(int(self.fold_in_epochs)):
            ops.lmf_half_step(plan, Y, X, A, self.learning_rate, self.regularization, 0 if seed is None else seed, FOLD_IN_ROUND | t,
                              K - 1)
        return X

    def _check_serving(self):
        if self.data.warm_start and self.filter_seen is False:
            raise ValueError('The model always filters seen items from results.')

    def _test_queries(self, test_users, start=0, stop=None):
        if self.data.warm_start:
            return self.fold_in()[start:stop]
        return super()._test_queries(test_users, start, stop)
