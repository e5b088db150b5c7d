"""LightFM with the WARP loss (polara/recommender/external/lightfm/lightfmwrapper.py, coldstart/models.py:260-298): the hybrid
matrix factorisation of Kula, "Metadata embeddings for user and item cold-start recommendations" (2015), trained with the
weighted approximate-rank pairwise loss of Weston, Bengio and Usunier (2011) and per-parameter adagrad.  The reference hands the
work to the third-party `lightfm` package; here the solver is the library's own (csrc/warp.hip), on the blocked schedule of
BPR (bpr.py) with the epoch's item order.

Rank k, fp64, C = k + 1 columns: P [n_users x C] with column k the constant 1, E_id [n_items x C] the items' identity
embeddings and E_lab [n_labels x C] the label embeddings, column k of both the bias.  The feature matrix is the reference's
`stack_features(..., add_identity=True, normalize=True)`: item i with m_i labels has the weight a_i = 1 / (1 + m_i) on its own
identity column and on each of its labels, so its representation is q_i = a_i E_id[i] + S_i with S = F_lab E_lab, and the scores
are P @ Q.T.  Without item features a_i = 1, there is no S, and the model is plain WARP-MF.

An epoch visits every stored positive once, in BPR's schedule order; up to `max_sampled` candidates from the positive's own item
part are scored against the LIVE factors and the first violator is used (the sample, the draw stream and the loss table are
spelled out in include/polara_hip.h).  The label embeddings are shared between items of different blocks: during a stratum they
are read-only (S is formed before it), the blocks add the label gradients of their own items into G, and after the stratum
every label takes ONE adagrad step on its summed gradient.  No atomics, no flags, bit-reproducible.  This is a bounded-staleness,
mini-batch treatment of the shared rows: the label embeddings take B steps per epoch, so `blocks` changes the algorithm and not
only the order (as it does for KPMF); with B = 1 the labels step once per epoch.

Against `lightfm`: fp64, every positive once per epoch, candidates inside the epoch's item part, a predrawn counter stream, the
rank estimate uses n_items - 1 although the draws come from a part, label steps per stratum, no regularisation, WARP and
adagrad only.  No equality with any build of `lightfm` is claimed.  Single process; no fold-in."""
from timeit import default_timer as timer

import numpy as np

from . import bpr
from .coldstart import (ItemColdStartEvaluationMixin, ItemColdStartRecommenderMixin, ItemColdStartSVDModelMixin, _frame_data,
                        check_image_memory, stack_features)
from .factor_serving import FactorQueriesMixin
from .models import RecommenderModel
from . import scoring

MAX_SAMPLED = 64            # the draw stream keeps 64 counters per entry


def default_blocks(nnz, n_users, n_items):
    """The B of `blocks=None`: BPR's rule (bpr.default_blocks).  UNMEASURED for this model: a WARP sample scores up to
    `max_sampled` candidates and, with features, every stratum adds two launches; tools/bench_warp.py times four values of B
    (DESIGN 8o), no rule was fitted to them."""
    return bpr.default_blocks(nnz, n_users, n_items)


def loss_table(n_items, max_sampled):
    """fp64 [D]: the weight of a violator found at draw t, min(10, log(max(1, floor((n_items - 1) / (t + 1))))) — NumPy on the
    host, so that the kernel needs no logarithm"""
    t = np.arange(int(max_sampled), dtype=np.float64)
    return np.minimum(10.0, np.log(np.maximum(1.0, np.floor((int(n_items) - 1) / (t + 1)))))


def initial_embeddings(n_users, n_items, n_labels, rank, seed=None):
    """(P0 [n_users x (k + 1)], E_id [n_items x (k + 1)], E_lab [n_labels x (k + 1)]): (rand - 0.5) / k draws for P, then E_id,
    then E_lab from `RandomState(seed)` (None: NumPy's global generator); the bias columns are 0, column k of P0 is 1"""
    rnds = np.random if seed is None else np.random.RandomState(seed)
    k = int(rank)
    P0, E0, L0 = np.ones((int(n_users), k + 1)), np.zeros((int(n_items), k + 1)), np.zeros((int(n_labels), k + 1))
    P0[:, :k] = (rnds.rand(int(n_users), k) - 0.5) / k
    E0[:, :k] = (rnds.rand(int(n_items), k) - 0.5) / k
    L0[:, :k] = (rnds.rand(int(n_labels), k) - 0.5) / k
    return P0, E0, L0


def feature_weights(one_hot):
    """SciPy one-hot [n_items x n_labels] -> (a fp64 [n_items] = 1 / (1 + labels of the item), F_lab = diag(a) one_hot as a
    canonical SciPy CSR): the label block of `stack_features(add_identity=True, normalize=True)`"""
    from scipy.sparse import csr_matrix
    F = csr_matrix(one_hot, dtype=np.float64)
    F.sum_duplicates()
    F.sort_indices()
    F.data[:] = 1.0
    a = 1.0 / (1.0 + np.diff(F.indptr).astype(np.float64))
    F.data[:] = np.repeat(a, np.diff(F.indptr))
    return a, F


def warp_fit(ops, matrix, rank, learning_rate, max_sampled, num_epochs, seed=None, blocks=None, reshuffle_items=True,
             item_features=None, init=None, history=None, iter_time=None, stats=None, comm=None):
    """`num_epochs` WARP sweeps over the stored entries of the ops-level canonical CSR `matrix` [n_users x n_items] (its values
    are ignored).  item_features: a SciPy one-hot matrix [n_items x n_labels] or None.  Returns the DEVICE blocks (P, E_id, E_lab,
    Q) of k + 1 columns (E_lab None without features).  seed: 32 unsigned bits; it seeds the initial embeddings, the item orders
    and the candidates.  history receives quiet / positives of every epoch.  init = (P0, E_id0, E_lab0) host arrays instead of
    the seeded draw.  The adagrad state starts at 1 and is kept over the epochs."""
    rank, D = int(rank), int(max_sampled)

    def begin(blocks, seed):
        n_users, n_items = (int(x) for x in matrix.shape)
        n_labels = 0
        if item_features is not None:
            if int(item_features.shape[0]) != n_items:
                raise ValueError('LightFM: features for %d items, the training matrix has %d' % (item_features.shape[0], n_items))
            n_labels = int(item_features.shape[1])
        candidate_bytes = int(matrix.nnz) * D * 4
        if hasattr(ops, 'free_bytes') and candidate_bytes > ops.free_bytes() / 2:
            raise MemoryError('LightFM: the candidates of an epoch (%d positives x %d draws) need %d bytes (%.2f GB), more than half '
                              'of the %.2f GB of free device memory' % (matrix.nnz, D, candidate_bytes, candidate_bytes / 1e9,
                                                                       ops.free_bytes() / 1e9))
        P0, E0, L0 = (np.asarray(a, dtype=np.float64)
                      for a in (initial_embeddings(n_users, n_items, n_labels, rank, seed) if init is None else init))
        if P0.shape != (n_users, rank + 1) or E0.shape != (n_items, rank + 1) or L0.shape != (n_labels, rank + 1):
            raise ValueError('LightFM: initial embeddings of shapes %s, %s, %s for (%d x %d), (%d x %d), (%d x %d)'
                             % (P0.shape, E0.shape, L0.shape, n_users, rank + 1, n_items, rank + 1, n_labels, rank + 1))
        P, E = ops.to_device(np.ascontiguousarray(P0)), ops.to_device(np.ascontiguousarray(E0))
        L = ops.to_device(np.ascontiguousarray(L0)) if item_features is not None else None
        state = tuple(None if X is None else ops.to_device(np.ones(tuple(X.shape))) for X in (P, E, L))
        table = loss_table(n_items, D)
        return ((P, E, L, candidate_bytes), lambda order: ops.warp_plan(matrix, blocks, order, item_features),
                lambda plan, epoch: ops.warp_epoch(plan, ops.warp_draw(plan, seed, epoch, D), table, P, E, state, learning_rate, L))

    (P, E, L, candidate_bytes), blocks, seed, plan, plan_time, (trained, quiet, draws) = bpr.pairwise_fit(
        'LightFM', ops, matrix, [('rank', rank, ops.warp_max_rank()), ('max_sampled', D, MAX_SAMPLED)], begin, num_epochs, seed, blocks,
        default_blocks, reshuffle_items, lambda counts: counts[1] / matrix.nnz if matrix.nnz else float('nan'), history, iter_time, comm)
    if plan is None:
        plan = ops.warp_plan(matrix, blocks, None, item_features)
    Q = ops.warp_representation(plan, E, L)
    if stats is not None:
        featured = item_features is not None
        stats.update(blocks=blocks, strata=blocks, launches_per_epoch=(3 * blocks + 3) if featured else (blocks + 2),
                     label_steps_per_epoch=blocks if featured else 0, reshuffle_items=bool(reshuffle_items), seed=seed,
                     epochs=len(trained), plan_time=plan_time, trained=trained, quiet=quiet, draws=draws, max_sampled=D,
                     candidate_bytes=candidate_bytes)
    return P, E, L, Q


class LightFMWrapper(FactorQueriesMixin, RecommenderModel):
    """lightfmwrapper.py:9-114 with the library's own solver.  `factors` holds four host fp64 arrays of k + 1 columns: users
    [P | 1], items the representation Q = a o E_id + F_lab E_lab (so that their product is the scores), f'{itemid}_identity'
    E_id and f'{itemid}_features' E_lab (no rows without item features).  `warp_history` is the share of quiet positives — those
    none of whose `max_sampled` candidates violated the margin — per epoch; `build_stats` the schedule, the trained and quiet
    samples and the draws per epoch and the size of the candidate buffer.  `item_features`: a frame or a dict whose cells are
    lists of labels (rows in item order), encoded with coldstart.stack_features; with array data also a SciPy one-hot matrix or
    one list of label ids per item.  `fit_params`: `epochs` (1, as LightFM's `fit`); `num_threads` is accepted and ignored.
    `blocks` (None: `default_blocks`) is the B of the blocked sweep — with item features it is also the number of steps the
    label embeddings take per epoch, each on one stratum's summed gradient: it changes the algorithm, not only the order —,
    `reshuffle_items` whether every epoch cuts the items along a fresh permutation.  Refused: every loss but 'warp', every
    schedule but 'adagrad', user features, item_identity=False, normalize_item_features=False, non-zero alphas, fit_partial,
    warm start, several processes.  A rank change invalidates the model."""

    def __init__(self, *args, item_features=None, user_features=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'LightFM'
        self._rank = 10
        self.fit_method = 'fit'
        self.fit_params = {}
        self.item_features = item_features
        self.item_features_labels = None
        self.item_alpha = 0.0
        self.item_identity = True
        self.normalize_item_features = True
        self.user_features = user_features
        self.user_features_labels = None
        self.user_alpha = 0.0
        self.user_identity = True
        self.normalize_user_features = True
        self.loss = 'warp'
        self.learning_schedule = 'adagrad'
        self.learning_rate = 0.05
        self.max_sampled = 10
        self.seed = 0
        self.blocks = None
        self.reshuffle_items = True
        self.factors = {}
        self.warp_history = None
        self.iterations_time = None
        self.build_stats = {}
        self._factors_dev = None            # (host user factors of `factors`, [P | 1] on the device, E_lab on the device)
        self.data.subscribe(self.data.on_change_event, self._clean_metadata)

    def _clean_metadata(self):
        super()._clean_metadata()
        self.item_features_labels = None

    def _check_settings(self):
        """what the solver does not do, refused before any work, each by name"""
        refusals = (
            (self.loss != 'warp', 'loss=%r (only \'warp\' is built)' % (self.loss,)),
            (self.learning_schedule != 'adagrad', 'learning_schedule=%r (only \'adagrad\' is built)' % (self.learning_schedule,)),
            (self.user_features is not None, 'user_features (only item features are built)'),
            (not self.item_identity, 'item_identity=False (every item keeps its identity embedding)'),
            (not self.normalize_item_features, 'normalize_item_features=False (feature rows are normalised)'),
            (float(self.item_alpha) != 0.0, 'item_alpha=%r (no regularisation is built)' % (self.item_alpha,)),
            (float(self.user_alpha) != 0.0, 'user_alpha=%r (no regularisation is built)' % (self.user_alpha,)),
            (self.fit_method != 'fit', 'fit_method=%r (only \'fit\' is built)' % (self.fit_method,)),
        )
        for refused, what in refusals:
            if refused:
                raise NotImplementedError('%s: %s' % (self.method, what))
        unknown = sorted(set(self.fit_params) - {'epochs', 'num_threads', 'verbose'})
        if unknown:
            raise NotImplementedError('%s: fit_params %s (epochs; num_threads and verbose are accepted and ignored)'
                                      % (self.method, ', '.join(unknown)))
        D = int(self.max_sampled)
        if D < 1 or D > MAX_SAMPLED:
            raise ValueError('%s: max_sampled %d outside 1..%d' % (self.method, D, MAX_SAMPLED))
        if int(self.rank) < 1 or int(self.rank) > self.ops.warp_max_rank():
            raise ValueError('%s: rank %d outside 1..%d' % (self.method, int(self.rank), self.ops.warp_max_rank()))

    def _check_serving(self):
        if self.data.warm_start:
            raise NotImplementedError('%s has no fold-in: warm start is not supported (the reference\'s wrapper raises '
                                      '\'Not supported by LightFM.\' too)' % self.method)

    def encode_item_features(self):
        """The one-hot matrix of the (training) items in the model's item order [n_items x n_labels] (SciPy CSR, ones): a
        frame under Polara's data model is re-indexed by the item index, a frame or dict next to array data is read row by
        row in item order, anything else goes through data.one_hot_csr."""
        d, f = self.data, self.item_features
        if _frame_data(d):
            index = d.index.itemid
            index = getattr(index, 'training', index)
            frame = f.reindex(index.old.values, fill_value=[])
            one_hot, self.item_features_labels = stack_features(frame)
            return one_hot
        if hasattr(f, 'columns') or isinstance(f, dict):
            one_hot, self.item_features_labels = stack_features(f)
            if one_hot.shape[0] != d.n_items:
                raise ValueError('features for %d items, the training matrix has %d' % (one_hot.shape[0], d.n_items))
            return one_hot
        return ItemColdStartSVDModelMixin.encode_item_features(self)

    def build(self):
        self._require_single_process_build()
        self._check_settings()
        ops = self.ops
        one_hot = self.encode_item_features() if self.item_features is not None else None
        train = self._training_device_csr()
        self.warp_history = []
        self.iterations_time = []
        stats = {}
        start = timer()
        P, E, L, Q = warp_fit(ops, train, self.rank, self.learning_rate, self.max_sampled, int(self.fit_params.get('epochs', 1)),
                              seed=self.seed, blocks=self.blocks, reshuffle_items=self.reshuffle_items, item_features=one_hot,
                              history=self.warp_history, iter_time=self.iterations_time, stats=stats)
        ops.synchronize()
        self._track(start)
        self.build_stats = stats
        if L is None:
            L = ops.to_device(np.zeros((0, int(self.rank) + 1)))
        self._set_factors(P, Q, kept=(L,), identity=E, features=L)

    def _extra_factors_device(self):
        L = self.factors[f'{self.data.fields.itemid}_features']
        return (self.ops.to_device(np.ascontiguousarray(L, dtype=np.float64)),)


class LightFMItemColdStart(ItemColdStartEvaluationMixin, ItemColdStartRecommenderMixin, LightFMWrapper):
    """coldstart/models.py:260-298: a cold item with m known labels has the representation q = (1 / m) sum_l E_lab[l] — no
    identity column, the row normalised, labels unknown to training dropped — and scores user u with q . [P | 1][u].  The queries
    are the cold items (one fp64 SpMM), the catalogue the rows of [P | 1] in descending-norm order, nothing is masked
    (scoring.recommend_dense).  Like the reference's, the lists range over ALL training users."""

    def __init__(self, *args, item_features=None, **kwargs):
        super().__init__(*args, item_features=item_features, **kwargs)
        if self.item_features is None:
            self.item_features = getattr(self.data, 'item_features', None)
        if self.item_features is None:
            raise ValueError('item cold start needs item features: pass item_features= or use a data object that has them')
        self.method = 'LightFM(cs)'
        self._user_image = None             # (host user factors, FactorImage of [P | 1] by norm, host order: position -> user)
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
        """(FactorImage of [P | 1] by descending row norm, host int64 order: catalogue position -> training user)"""
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

    def _cold_features_device(self):
        """the cold items' one-hot rows over the training labels, each divided by its number of labels, as a device CSR"""
        key = self.item_features_labels
        if self._cold_dev is None or self._cold_dev[0] is not key:
            F = self._cold_one_hot().tocsr().astype(np.float64)
            F.sum_duplicates()
            F.sort_indices()
            counts = np.diff(F.indptr)
            F.data[:] = np.repeat(1.0 / np.maximum(counts, 1), counts)
            self._cold_dev = (key, self.ops.csr(F.indptr, F.indices, F.data, F.shape))
        return self._cold_dev[1]

    def _cold_queries_device(self):
        """q = F_cold E_lab on the device (coldstart/models.py:263-280)"""
        self._user_factors_block()
        L = self._factors_dev[2]
        F = self._cold_features_device()
        if F.shape[1] != L.shape[0]:
            raise ValueError('cold item features over %d labels, the embeddings over %d' % (F.shape[1], L.shape[0]))
        return self.ops.spmm(F, L)
