"""The factorisation model with side features (polara/recommender/external/turi/turiwrapper.py, method 'TCF'): rating
regression with a global mean, user and item biases, linear terms for the user and item side features and factorised
interactions.  The reference hands the work to the third-party `turicreate` package; here the solver is the library's own
(csrc/fm.hip), on PMF's blocked schedule (pmf.py) in PMF's order: no per-epoch reshuffle, `blocks=1` is the serial sweep.

Rank k, fp64, C = k + 2 columns, so that one dot product is the whole prediction:

    P  [n_users   x C]  user identity rows:  factors | bias          | 1
    LU [n_ulabels x C]  user label rows:     factors | linear weight | 0
    E  [n_items   x C]  item identity rows:  factors | 1             | bias
    LI [n_ilabels x C]  item label rows:     factors | 0             | linear weight

    pt_u = aU_u P_u + sum_m FU_um LU_m,    qt_i = aI_i E_i + sum_l FI_il LI_l,    yhat(u, i) = mu + pt_u . qt_i
                                                                                           = mu + b_u + b_i + <p_u, q_i>

with b and p, q the bias and factor parts of the two representations.  The model passes a = 1 and F = one-hot, Turi's
semantics; with `normalize_side_features=True` a row with m labels weighs its identity row and each label by 1 / (1 + m), as
LightFM does (warp.feature_weights) — the constant column is then a too.  The loss of a stored rating r is
(yhat - r)^2 / 2 + lambda_f / 2 |factor columns touched|^2 + lambda_lin / 2 |bias columns touched|^2.  With
`side_data_factorization=False` the label factor columns stay 0 and only the labels' linear weights are stepped.

NOT a full factorisation machine: the interactions INSIDE one side (user id x user labels, item id x item labels, label x
label of one side) are dropped.  For a fixed user the dropped user-side term is constant over the items, so it cannot change a
top-k list; the dropped item-side term is a per-item offset, which the item bias and the item labels' linear weights model on
their own.  What remains keeps the blocks of a stratum independent.

The label rows are shared between blocks: during a stratum they are read-only (their images are formed before it), the
blocks add their rows' label gradients and sample counts into G, and after the stratum every label that was sampled takes
ONE step on its summed gradient (plus lambda x its sample count x itself).  No atomics, bit-reproducible.  The label rows
therefore take B steps per epoch: with features `blocks` changes the algorithm and not only the order (as it does for
LightFM here); with B = 1 the labels step once per epoch.

Step rules: x <- x - step * adj(g); the state of adj starts at 0 and is KEPT over the epochs.  solver='sgd': adj(g) = g;
'adagrad' ('auto') with adagrad_momentum_weighting=None: PMF's adagrad; with a float gamma in (0, 1): PMF's rmsprop with that
gamma — Turi's "momentum-weighted" adagrad is of this form.  sgd_step_size=0, Turi's "choose for me", is a stated default of
THIS library, not Turi's line search: 0.05 with an adjuster, 0.005 (PMF's rate) without.

No equality with any build of turicreate is claimed.  Single process; no fold-in."""
import math
from timeit import default_timer as timer

import numpy as np

from . import pmf, scoring
from .coldstart import (ItemColdStartEvaluationMixin, ItemColdStartRecommenderMixin, ItemColdStartSVDModelMixin, _frame_data,
                        check_image_memory, stack_features)
from .factor_serving import FactorQueriesMixin
from .models import RecommenderModel

SOLVERS = ('auto', 'adagrad', 'sgd')
DEFAULT_STEP = {True: 0.05, False: 0.005}          # sgd_step_size=0: with an adjuster / without (PMF's learn_rate)


def default_blocks(nnz, n_users, n_items):
    """The B of `blocks=None`: PMF's rule (pmf.default_blocks).  UNMEASURED for this model: a sample reads two more rows and
    updates two rows of G, and with features every stratum adds two launches per side; tools/bench_fm.py times the default and
    B = 1 024, no rule was fitted to them."""
    return pmf.default_blocks(nnz, n_users, n_items)


def side_features(one_hot, normalize=False):
    """SciPy one-hot [n_rows x n_labels] -> (a fp64 [n_rows], F = diag(a) one_hot as a canonical SciPy CSR): a = 1, or with
    `normalize` LightFM's 1 / (1 + labels of the row) (warp.feature_weights)"""
    from scipy.sparse import csr_matrix
    if normalize:
        from .warp import feature_weights
        return feature_weights(one_hot)
    F = csr_matrix(one_hot, dtype=np.float64)
    F.sum_duplicates()
    F.sort_indices()
    F.data[:] = 1.0
    return np.ones(F.shape[0]), F


def initial_parameters(n_users, n_items, n_ulabels, n_ilabels, rank, seed=None):
    """(P [n_users x (k + 2)], E [n_items x (k + 2)], LU [n_ulabels x (k + 2)], LI [n_ilabels x (k + 2)]): N(0, 0.1^2) factor
    columns drawn for P, then E, then LU, then LI from `RandomState(seed)` (None: NumPy's global generator); biases and linear
    weights 0; the constant column of P (k + 1) and of E (k) is 1"""
    rnds = np.random if seed is None else np.random.RandomState(seed)
    k = int(rank)
    blocks = []
    for n in (n_users, n_items, n_ulabels, n_ilabels):
        X = np.zeros((int(n), k + 2))
        X[:, :k] = rnds.normal(scale=0.1, size=(int(n), k))
        blocks.append(X)
    blocks[0][:, k + 1] = 1.0
    blocks[1][:, k] = 1.0
    return tuple(blocks)


def step_rule(solver='auto', adagrad_momentum_weighting=0.9, sgd_step_size=0, what='TCF'):
    """(adjust, gamma, step) of the model's settings: adjust None / 'adagrad' / 'rmsprop' as the sweep names them"""
    if solver not in SOLVERS:
        raise NotImplementedError('%s: solver=%r is not implemented (%s)' % (what, solver, ', '.join(repr(s) for s in SOLVERS)))
    adjust, gamma = None, pmf.RMSPROP_GAMMA
    if solver != 'sgd':
        adjust = 'adagrad'
        if adagrad_momentum_weighting is not None:
            gamma = float(adagrad_momentum_weighting)
            if not 0.0 < gamma < 1.0:
                raise ValueError('%s: adagrad_momentum_weighting %r outside (0, 1) (None: plain adagrad)' % (what, adagrad_momentum_weighting))
            adjust = 'rmsprop'
    step = float(sgd_step_size)
    if step < 0:
        raise ValueError('%s: sgd_step_size %r is negative' % (what, sgd_step_size))
    if step == 0:
        step = DEFAULT_STEP[adjust is not None]
    return adjust, gamma, step


def fm_fit(ops, matrix, rank, num_epochs, mean, regularization=1e-10, linear_regularization=1e-10, adjust='rmsprop',
           gamma=pmf.RMSPROP_GAMMA, step=0.05, seed=None, blocks=None, user_features=None, item_features=None, normalize=False,
           label_factors=True, init=None, history=None, iter_time=None, stats=None, comm=None):
    """`num_epochs` sweeps over the stored ratings of the ops-level canonical CSR `matrix` [n_users x n_items] around the
    global mean `mean`.  user_features / item_features: SciPy one-hot matrices [n_rows x n_labels] or None.  Returns the DEVICE
    blocks (P, E, LU, LI, Pt, Qt) of k + 2 columns: the four parameter blocks (LU / LI None without features on their side)
    and the two representations, whose product is yhat - mean.  init = (P0, E0, LU0, LI0) host arrays instead of the seeded
    draw.  history receives the RMSE of every epoch (from the errors before each update); one double is read back per epoch."""
    if comm is not None and getattr(comm, 'world', 1) > 1:
        raise NotImplementedError('TCF: multi-process builds are not supported (comm.world = %d)' % comm.world)
    n_users, n_items = (int(x) for x in matrix.shape)
    rank = int(rank)
    if rank < 1 or rank > ops.fm_max_rank():
        raise ValueError('TCF: rank %d outside 1..%d' % (rank, ops.fm_max_rank()))
    if blocks is None:
        blocks = default_blocks(matrix.nnz, n_users, n_items)
    blocks = int(blocks)
    if blocks < 1 or blocks > min(n_users, n_items):
        raise ValueError('TCF: %d blocks for %d users and %d items (1 .. min of the two)' % (blocks, n_users, n_items))
    sides = (('user', user_features, n_users), ('item', item_features, n_items))
    for side, features, n in sides:
        if features is not None and int(features.shape[0]) != n:
            raise ValueError('TCF: features for %d %ss, the training matrix has %d' % (features.shape[0], side, n))
    n_labels = [0 if features is None else int(features.shape[1]) for _, features, _ in sides]
    start = timer()
    plan = ops.fm_plan(matrix, blocks, user_features, item_features, normalize)
    plan_time = timer() - start
    init = initial_parameters(n_users, n_items, n_labels[0], n_labels[1], rank, seed) if init is None else init
    host = [np.ascontiguousarray(x, dtype=np.float64) for x in init]
    shapes = [(n, rank + 2) for n in (n_users, n_items, n_labels[0], n_labels[1])]
    if [x.shape for x in host] != shapes:
        raise ValueError('TCF: initial parameters of shapes %s for %s' % ([x.shape for x in host], shapes))
    if not label_factors:                                             # the label factor columns stay 0 and are never stepped
        host[2][:, :rank] = 0.0
        host[3][:, :rank] = 0.0
    P, E = ops.to_device(host[0]), ops.to_device(host[1])
    LU = ops.to_device(host[2]) if user_features is not None else None
    LI = ops.to_device(host[3]) if item_features is not None else None
    state = tuple(None if X is None else ops.zeros(*tuple(X.shape)) for X in (P, E, LU, LI)) if adjust else None
    work = tuple(None if f is None else ops.empty(n, rank + 2 + extra)
                 for _, f, n in sides for extra in (0, 1))                         # SU, GU, SI, GI
    nnz, epochs = int(plan['nnz']), 0
    for _ in range(int(num_epochs)):
        start = timer()
        sse = ops.fm_epoch(plan, mean, P, E, LU, LI, state, step, regularization, linear_regularization, adjust=adjust, gamma=gamma,
                           work=work, label_factors=label_factors, smoothing=pmf.SMOOTHING)
        new_err = float(sse[0].item())                      # the epoch's one host read
        epochs += 1
        if history is not None:
            history.append(math.sqrt(new_err / nnz) if nnz else float('nan'))
        if iter_time is not None:
            iter_time.append(timer() - start)
    if stats is not None:
        featured = sum(f is not None for _, f, _ in sides)
        stats.update(pmf.schedule_stats(ops.to_host(plan['block_ptr']), blocks), epochs=epochs, plan_time=plan_time,
                     launches_per_epoch=blocks * (1 + 2 * featured) + featured + 1, label_steps_per_epoch=blocks if featured else 0,
                     adjust=adjust, gamma=gamma, step=step, user_labels=n_labels[0], item_labels=n_labels[1])
    return P, E, LU, LI, ops.fm_representation(plan, 'user', P, LU), ops.fm_representation(plan, 'item', E, LI)


class TuriFactorizationRecommender(FactorQueriesMixin, RecommenderModel):
    """turiwrapper.py:6-169 with the library's own solver; every attribute of the reference's `__init__` keeps its name and its
    default.  `factors` holds host fp64 arrays of k + 2 columns: users the representation Pt, items Qt (their product is
    yhat - global_mean), f'{itemid}_identity' E, f'{itemid}_features' LI, f'{userid}_identity' P and f'{userid}_features' LU
    (no rows without side information on that side).  `item_side_info` / `user_side_info`: a frame or a dict whose cells are
    lists of labels (rows in item / user order), encoded with coldstart.stack_features; with array data also a SciPy one-hot
    matrix.  `blocks` (None: `default_blocks`) is the B of the blocked sweep — with side information it is also the number of
    steps the label rows take per epoch: it changes the algorithm, not only the order.  `normalize_side_features`: LightFM's
    1 / (1 + m) weights instead of Turi's sum.  `rmse_history` is the training RMSE per epoch, from the errors before each update.
    The model is this module's (see its docstring): interactions inside one side are dropped, so it is not a full
    factorisation machine, and nothing is claimed about turicreate's numbers.  Refused by name: ranking_optimization=True,
    with_data_feedback=False (Turi then ranks), binary_target=True, every solver but 'auto', 'adagrad' and 'sgd', a non-empty
    other_tc_params, warm start, several processes.  A rank change invalidates the model."""

    def __init__(self, *args, item_side_info=None, user_side_info=None, **kwargs):
        self.item_side_info = item_side_info
        self.user_side_info = user_side_info
        super().__init__(*args, **kwargs)
        self._rank = 10
        self.method = 'TCF'
        self.side_data_factorization = True
        self.seed = 61
        self.binary_target = False
        self.solver = 'auto'
        self.max_iterations = 25
        self.regularization = 1e-10
        self.linear_regularization = 1e-10
        self.adagrad_momentum_weighting = 0.9
        self.sgd_step_size = 0
        self.ranking_optimization = False
        self.ranking_regularization = 0.25
        self.unobserved_rating_value = None
        self.num_sampled_negative_examples = 4
        self.with_data_feedback = True
        self.other_tc_params = {}
        self.blocks = None
        self.normalize_side_features = False
        self.item_features_labels = None
        self.user_features_labels = None
        self.factors = {}
        self.rmse_history = None
        self.iterations_time = None
        self.build_stats = {}
        self.global_mean = None
        self._factors_dev = None            # (host user factors of `factors`, Pt on the device, LI on the device)
        self.data.subscribe(self.data.on_change_event, self._clean_metadata)

    @property
    def num_factors(self):
        return self.rank

    @num_factors.setter
    def num_factors(self, new_value):
        self.rank = new_value

    @property
    def item_features(self):
        """the item side information under the name the cold-start mixins read it by"""
        return self.item_side_info

    def _clean_metadata(self):
        super()._clean_metadata()
        self.item_features_labels = self.user_features_labels = None

    def _check_settings(self):
        """what the solver does not do, refused before any work, each by name"""
        refusals = (
            (bool(self.ranking_optimization), 'ranking_optimization=True (only the rating regression is built)'),
            (not self.with_data_feedback, 'with_data_feedback=False (without a target Turi ranks; only the rating regression is built)'),
            (bool(self.binary_target), 'binary_target=True (only the squared error is built)'),
            (bool(self.other_tc_params), 'other_tc_params=%r (there is no turicreate to hand them to)' % (self.other_tc_params,)),
        )
        for refused, what in refusals:
            if refused:
                raise NotImplementedError('%s: %s' % (self.method, what))
        rule = step_rule(self.solver, self.adagrad_momentum_weighting, self.sgd_step_size, self.method)
        if int(self.rank) < 1 or int(self.rank) > self.ops.fm_max_rank():
            raise ValueError('%s: rank %d outside 1..%d' % (self.method, int(self.rank), self.ops.fm_max_rank()))
        for name in ('regularization', 'linear_regularization'):
            if not float(getattr(self, name)) >= 0.0:
                raise ValueError('%s: %s %r is negative' % (self.method, name, getattr(self, name)))
        return rule

    def _check_serving(self):
        if self.data.warm_start:
            raise NotImplementedError('%s has no fold-in: warm start is not supported (the reference\'s wrapper raises too)'
                                      % self.method)

    def _encode_side(self, side):
        """(one-hot SciPy CSR [n_rows x n_labels] in the model's row order, labels) of one side's information: a frame under
        Polara's data model is re-indexed by the side's index, a frame or dict next to array data is read row by row, a SciPy
        matrix (or anything data.one_hot_csr takes) is used as it is"""
        d = self.data
        info = self.user_side_info if side == 'user' else self.item_side_info
        n = d.n_users if side == 'user' else d.n_items
        if _frame_data(d):
            index = getattr(d.index, d.fields.userid if side == 'user' else d.fields.itemid)
            index = getattr(index, 'training', index)
            return stack_features(info.reindex(index.old.values, fill_value=[]))
        if hasattr(info, 'columns') or isinstance(info, dict):
            one_hot, labels = stack_features(info)
        elif side == 'item':
            one_hot = ItemColdStartSVDModelMixin.encode_item_features(self)          # (the labels some training item carries)
            labels = self.item_features_labels
        else:
            from .data import one_hot_csr
            one_hot = one_hot_csr(info, n_rows=n).tocsr()
            labels = np.arange(one_hot.shape[1])
        if one_hot.shape[0] != n:
            raise ValueError('%s: side information for %d %ss, the training matrix has %d' % (self.method, one_hot.shape[0], side, n))
        return one_hot, labels

    def build(self):
        self._require_single_process_build()
        adjust, gamma, step = self._check_settings()
        ops = self.ops
        FU = FI = None
        if self.user_side_info is not None:
            FU, self.user_features_labels = self._encode_side('user')
        if self.item_side_info is not None:
            FI, self.item_features_labels = self._encode_side('item')
        train = self._training_device_csr()
        values = ops.csr_values_host(train)
        self.global_mean = float(np.mean(values)) if len(values) else 0.0
        self.rmse_history = []
        self.iterations_time = []
        stats = {}
        start = timer()
        P, E, LU, LI, Pt, Qt = fm_fit(ops, train, self.rank, self.max_iterations, self.global_mean, self.regularization,
                                      self.linear_regularization, adjust, gamma, step, seed=self.seed, blocks=self.blocks,
                                      user_features=FU, item_features=FI, normalize=self.normalize_side_features,
                                      label_factors=self.side_data_factorization, history=self.rmse_history,
                                      iter_time=self.iterations_time, stats=stats)
        ops.synchronize()
        self._track(start)
        self.build_stats = stats
        empty = lambda: ops.to_device(np.zeros((0, int(self.rank) + 2)))
        LU, LI = (empty() if LU is None else LU), (empty() if LI is None else LI)
        self._set_factors(Pt, Qt, kept=(LI,), identity=E, features=LI)
        userid = self.data.fields.userid
        self.factors[f'{userid}_identity'] = ops.to_host(P)
        self.factors[f'{userid}_features'] = ops.to_host(LU)

    def _extra_factors_device(self):
        L = self.factors[f'{self.data.fields.itemid}_features']
        return (self.ops.to_device(np.ascontiguousarray(L, dtype=np.float64)),)

    def predict(self, users, items):
        """yhat of (user, item) pairs in the model's numbering, on the host from `factors`"""
        P, Q = self.factors[self.data.fields.userid], self.factors[self.data.fields.itemid]
        users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
        return self.global_mean + np.einsum('ij,ij->i', P[users], Q[items])

    def evaluate_rmse(self):
        """turiwrapper.py:164-169: the RMSE of the predictions on the holdout pairs, on the host from `factors`"""
        self._check_serving()
        if not self._is_ready:
            self.build()
        hold = self.data.test.holdout
        fields = self.data.fields
        if hasattr(hold, 'columns'):
            u, i, r = (hold[name].values for name in (fields.userid, fields.itemid, fields.feedback))
        else:
            u, i, r = hold
        err = self.predict(u, i) - np.asarray(r, dtype=np.float64)
        return float(np.sqrt(np.mean(err * err)))


class TuriFactorizationItemColdStart(ItemColdStartEvaluationMixin, ItemColdStartRecommenderMixin, TuriFactorizationRecommender):
    """The reference's ColdStartRecommendationsMixin (turiwrapper.py:178-203) on the device: a cold item has no identity row,
    so its representation is q = w (e_k + sum_l LI[l]) over its labels known to training — e_k the constant column an identity
    row would carry, so that the user bias counts in the ranking of the users; w the weight of training: 1, or 1 / (1 + m) with
    `normalize_side_features` — and it scores user u with q . Pt[u].  The queries are the cold items (one fp64 SpMM), the
    catalogue the rows of Pt in descending-norm order, nothing is masked (scoring.recommend_dense).  The lists range over ALL
    training users."""

    def __init__(self, *args, item_side_info=None, **kwargs):
        super().__init__(*args, item_side_info=item_side_info, **kwargs)
        if self.item_side_info is None:
            self.item_side_info = getattr(self.data, 'item_features', None)
        if self.item_side_info is None:
            raise ValueError('item cold start needs item side information: pass item_side_info= or use a data object that has it')
        self.method = 'TCF(cs)'
        self._user_image = None             # (host user factors, FactorImage of Pt by norm, host order: position -> user)
        self._cold_dev = None
        self.data.subscribe(self.data.on_update_event, self._clean_cold_items)

    def _clean_metadata(self):
        super()._clean_metadata()
        self._user_image = self._cold_dev = None

    def _clean_cold_items(self):
        self._cold_dev = None

    _cold_one_hot = ItemColdStartSVDModelMixin._cold_one_hot

    def build(self, *args, **kwargs):
        super().build(*args, **kwargs)
        self._cold_dev = None
        self._user_factors_device()

    def _user_factors_device(self):
        """(FactorImage of Pt by descending row norm, host int64 order: catalogue position -> training user)"""
        P = self.factors.get(self.data.fields.userid, None)
        if P is None:
            raise ValueError('%s: no user factors (build the model first)' % self.method)
        cached = self._user_image
        if cached is not None and cached[0] is P:
            return cached[1], cached[2]
        ops = self.ops
        if hasattr(ops, 'free_bytes'):
            check_image_memory(P.shape[0], P.shape[1], ops.free_bytes())
        order, Xs = self._rows_by_norm(self._user_factors_block())
        image = scoring.FactorImage(ops, Xs)
        self._user_image = (P, image, order)
        return image, order

    def cold_weights(self, one_hot):
        """w of every row of a cold one-hot CSR: the weight its labels (and its constant) had in training"""
        counts = np.diff(one_hot.indptr).astype(np.float64)
        return 1.0 / (1.0 + counts) if self.normalize_side_features else np.ones(len(counts))

    def _cold_features_device(self):
        """(the cold items' one-hot rows over the training labels, weighted as in training, as a device CSR; the weights)"""
        key = self.item_features_labels
        if self._cold_dev is None or self._cold_dev[0] is not key:
            F = self._cold_one_hot().tocsr().astype(np.float64)
            F.sum_duplicates()
            F.sort_indices()
            w = self.cold_weights(F)
            F.data[:] = np.repeat(w, np.diff(F.indptr))
            self._cold_dev = (key, self.ops.csr(F.indptr, F.indices, F.data, F.shape), self.ops.to_device(w))
        return self._cold_dev[1], self._cold_dev[2]

    def _cold_queries_device(self):
        """q = F_cold LI on the device, with the constant column k set to the row's weight"""
        self._user_factors_block()
        L = self._factors_dev[2]
        F, w = self._cold_features_device()
        if F.shape[1] != L.shape[0]:
            raise ValueError('cold item features over %d labels, the embeddings over %d' % (F.shape[1], L.shape[0]))
        q = self.ops.spmm(F, L)
        q[:, int(self.rank)] = w
        return q
