"""Item cold start (polara/recommender/coldstart/models.py): for items nobody has rated yet, which training users will want
them?  The four factor models of the reference — PureSVD(cs), PureSVD(cs)-s, HybridSVD(cs), HybridSVD(cs)-s — and the
most-active-users baseline MP(cs), on top of this package's SVDModel / HybridSVD.

A factor model is its parent's model built with the user factors kept, plus the map from item features into the latent
space: W = F_train^T P (P: the item factors V, or HybridSVD's right projector vr) and G = pinv(W^T W).  A cold item with the
one-hot feature row x scores user u with (x W) G . (U diag(sigma))[u].  The scoring pass is the package's usual one turned
round: the QUERIES are the cold items (dense rank-r rows E = (F_cold W) G: one SpMM and one small product), the CATALOGUE is
the users (rows of U diag(sigma) in descending-norm order, a scoring.FactorImage), nothing is masked
(scoring.recommend_dense).  The [n_cold x n_users] score block of the reference (coldstart/models.py:209-222) is never
materialised.  Single process."""
from collections import OrderedDict

import numpy as np

from . import scoring
from .models import HybridSVD, RecommenderModel, ScaledMatrixMixin, SVDModel, get_default

IMAGE_BYTES_PER_ELEMENT = 8 + 8 + 4 + 4 + 4      # U diag(sigma) unordered and ordered (fp64), packed fragments, fp32 image, q20 image (fp32-sized bound)


def user_image_bytes(n_users, rank):
    """Device bytes the users' side of a cold-start pass takes while it is built (upper estimate): the fp64 block
    U diag(sigma) before and after ordering and the three fp32-sized images of scoring.FactorImage, rows padded to 32
    columns."""
    cols = -(-(int(rank) + 1) // 32) * 32
    return int(n_users) * cols * IMAGE_BYTES_PER_ELEMENT


def check_image_memory(n_users, rank, free_bytes):
    """The guard of the users' image (like hybrid.check_factor_memory): it must fit in half of the free device memory."""
    need = user_image_bytes(n_users, rank)
    if need > free_bytes / 2:
        raise MemoryError('item cold start: the device image of the user factors (%d users x rank %d) needs %d bytes '
                          '(%.2f GB), more than half of the %.2f GB of free device memory'
                          % (n_users, rank, need, need / 1e9, free_bytes / 1e9))
    return need


def stack_features(features, labels=None):
    """`polara.lib.similarity.stack_features(features, labels=labels, normalize=False, stacked_index=False)` restated on
    the host without pandas operations: `features` is a frame (or a dict of columns) whose cells are lists of labels.  Every
    column gets its own block of one-hot columns, a label's number is the order in which the column first shows it (a cell
    is read as `set(cell)`, like feature2sparse, lib/similarity.py:255-298); with `labels` (the dicts a previous call
    returned) unknown labels are dropped.  Returns (SciPy CSR [n_rows x n_labels] of ones, {column: {label: number}})."""
    from scipy.sparse import csr_matrix, hstack
    columns = list(features.columns) if hasattr(features, 'columns') else list(features.keys())
    mats, out_labels = [], OrderedDict()
    for col in columns:
        cells = [set(c) for c in (features[col].values if hasattr(features[col], 'values') else features[col])]
        if labels:
            lbl = labels[col]
            rows = [[lbl[x] for x in c if x in lbl] for c in cells]
        else:
            lbl = {}
            rows = [[lbl.setdefault(x, len(lbl)) for x in c] for c in cells]
        indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
        indices = np.fromiter((i for r in rows for i in r), dtype=np.int64, count=int(indptr[-1]))
        mats.append(csr_matrix((np.ones(len(indices)), indices, indptr), shape=(len(cells), len(lbl))))
        out_labels[col] = dict(lbl)
    stacked = hstack(mats, format='csr', dtype=np.float64) if mats else csr_matrix((0, 0))
    stacked.sort_indices()
    return stacked, out_labels


def _frame_data(data):
    return hasattr(getattr(data, 'index', None), 'itemid')        # Polara's RecommenderData (pandas index tables)


class ItemColdStartEvaluationMixin:
    """coldstart/models.py:13-18: nothing is seen in cold start; the key of a prediction is the cold item, its target the
    user."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.filter_seen = False
        self._prediction_key = '{}_cold'.format(self.data.fields.itemid)
        self._prediction_target = self.data.fields.userid

    def _cold_shape(self):
        """(cold items, training users)"""
        d = self.data
        if _frame_data(d):
            return int(d.index.itemid.cold_start.shape[0]), int(d.index.userid.training.shape[0])
        return int(d.n_cold_items), int(d.n_users)

    def _representative_users(self):
        r = getattr(self.data, 'representative_users', None)
        if r is None:
            return None
        return np.asarray(r.new.values if hasattr(r, 'new') else r, dtype=np.int64)

    def evaluate(self, metric_type='all', topk=None, not_rated_penalty=None, switch_positive=None,
                 ignore_feedback=False, simple_rates=False, on_feedback_level=None):
        """models.py:408-485 with the roles swapped: rows of the lists are cold items, entries are users, the catalogue
        of the coverage is the training users."""
        holdout = self.data.test.holdout
        if hasattr(holdout, 'columns'):              # a pandas frame: Polara's data model is in use
            from polara.recommender.models import RecommenderModel as _Ref
            return _Ref.evaluate(self, metric_type=metric_type, topk=topk, not_rated_penalty=not_rated_penalty,
                                 switch_positive=switch_positive, ignore_feedback=ignore_feedback,
                                 simple_rates=simple_rates, on_feedback_level=on_feedback_level)
        from . import evaluation
        if holdout is None:
            raise ValueError('evaluate() needs a holdout')
        if int(topk or 0) > self.topk:
            self.topk = topk
        recs = self.recommendations[:, :topk]
        users, cold, fdbk = holdout                  # sorted by cold item (data.ItemColdStartArrayData)
        fb = None if fdbk is None else np.asarray(fdbk, dtype=np.float64)
        return evaluation.evaluate(recs, np.asarray(cold), np.asarray(users), fb, self._cold_shape()[1],
                                   metric_type=metric_type, not_rated_penalty=not_rated_penalty,
                                   switch_positive=switch_positive or self.switch_positive,
                                   ignore_feedback=ignore_feedback, simple_rates=simple_rates,
                                   holdout_size=self.data.holdout_size,
                                   ndcg_alternative=get_default('ndcg_alternative'))


class ItemColdStartRecommenderMixin:
    """coldstart/models.py:21-52 without the chunk loop: one device pass over all cold items."""

    def get_recommendations(self):
        if self.verify_integrity:
            self.verify_data_integrity()
        ops = self.ops
        n_cold, n_users = self._cold_shape()
        if self.topk > n_users:
            raise ValueError('kth(=%d) out of bounds (%d)' % (n_users - self.topk, n_users))
        self._recs_dev = None
        if n_cold == 0:
            return np.empty((0, self.topk), dtype=np.int64)
        image, order = self._user_factors_device()
        E = self._cold_queries_device()
        stats = {}
        recs_dev = scoring.recommend_dense(ops, image, E, self.topk, stats=stats if self.collect_recommend_stats else None)
        self.recommend_stats = stats
        return self._external_ids(recs_dev, order)          # catalogue positions -> training user ids

    def slice_recommendations(self, cold_item_meta=None, start=0, stop=None):
        """coldstart/models.py:133-146, 209-222: the dense fp64 scores of cold items [start, stop) against every training
        user (in user id order).  Kept for consumers of score blocks; `get_recommendations` does not go through here."""
        n_cold = self._cold_shape()[0]
        stop = n_cold if stop is None else min(stop, n_cold)
        image, order = self._user_factors_device()
        E = self._cold_queries_device()[start:stop].contiguous()
        scores = self.ops.to_host(self.ops.dense_scores(image.V, E))
        out = np.empty_like(scores)
        out[:, order] = scores
        return out


class ItemColdStartSVDModelMixin:
    """coldstart/models.py:149-222: the feature embeddings W, the transform helper G = pinv(W^T W) and their life cycle
    (rank truncation, data events), plus the device state of the pass."""

    def __init__(self, *args, item_features=None, **kwargs):
        super().__init__(*args, **kwargs)
        features = item_features if item_features is not None else getattr(self.data, 'item_features', None)
        if features is None:
            raise ValueError('item cold start needs item features: pass item_features= or use a data object that has them')
        self.item_features = features
        self.item_features_labels = None
        self._item_features_transform_helper = None      # G = pinv(W^T W), [rank x rank]
        self._keep_user_factors_on_device = True
        self._user_factors_dev = None           # (host U of `factors`, the same block on the device) from the last build
        self._user_image = None                 # (U, sigma of `factors`, FactorImage of the users, host order: position -> user)
        self._features_dev = None               # (W of `factors`, helper, W on the device, helper on the device)
        self._cold_dev = None                   # (labels / data features it was made from, device CSR arrays of the cold items)
        self.data.subscribe(self.data.on_change_event, self._clean_metadata)
        self.data.subscribe(self.data.on_update_event, self._clean_cold_items)

    def _clean_metadata(self):
        self.item_features_labels = None
        self._user_factors_dev = self._user_image = self._features_dev = self._cold_dev = None

    def _clean_cold_items(self):
        self._cold_dev = None

    @property
    def item_features_embeddings(self):
        return self.factors.get(f'{self.data.fields.itemid}_features', None)

    # ---- rank truncation (coldstart/models.py:169-183) ----------------------------------------------------------------
    def _round_item_features_transform(self):
        """After the factors were cut to a smaller rank: G is recomputed from the truncated W.  Without embeddings (the
        rank grew and the factors were dropped) there is no helper either; a helper that is not larger than the factors
        means the call was no reduction — the reference's ValueError."""
        W = self.item_features_embeddings
        if W is None:
            self._item_features_transform_helper = None
            return
        if self._item_features_transform_helper.shape[0] <= W.shape[1]:
            raise ValueError('Unable to round: the rank of factors is not lower than the rank of transform!')
        self.update_item_features_transform()

    def _check_reduced_rank(self, rank):
        super()._check_reduced_rank(rank)
        self._round_item_features_transform()

    # ---- features ----------------------------------------------------------------------------------------------------
    def encode_item_features(self):
        """The one-hot matrix of the training items in the model's item order [n_items x n_labels] (SciPy CSR) over the
        labels that some training item carries."""
        d = self.data
        if _frame_data(d):
            training_items = d.index.itemid.training.old.values
            frame = self.item_features.reindex(training_items, fill_value=[])
            one_hot, self.item_features_labels = stack_features(frame)
            return one_hot
        from .data import one_hot_csr
        F = one_hot_csr(self.item_features, n_rows=d.n_items)
        self.item_features_labels = np.flatnonzero(np.diff(F.tocsc().indptr) > 0)       # labels known to training
        return F[:, self.item_features_labels].tocsr()

    def _cold_one_hot(self):
        """The one-hot matrix of the cold items over the training labels (SciPy CSR); a cold item's unknown labels are
        not in it."""
        d = self.data
        if self.item_features_labels is None:
            raise ValueError('%s: no feature labels (build the model first)' % self.method)
        if _frame_data(d):
            frame = self.item_features.reindex(d.index.itemid.cold_start.old.values, fill_value=[])
            return stack_features(frame, labels=self.item_features_labels)[0]
        return d.cold_item_features[:, self.item_features_labels].tocsr()

    def update_item_features_transform(self):
        """G = pinv(W^T W) on the host in fp64 with NumPy's default cut-off (part of the contract: rank x rank)."""
        W = self.item_features_embeddings
        self._item_features_transform_helper = np.linalg.pinv(W.T @ W)

    def prepare_item_features_transformation(self):
        """W = F_train^T P goes into `factors` (so that a rank reduction cuts its columns with the others), then G."""
        W = self.compute_item_features_mapping(self.encode_item_features())
        self.factors[f'{self.data.fields.itemid}_features'] = np.ascontiguousarray(W)
        self.update_item_features_transform()

    def build(self, *args, **kwargs):
        self._require_single_process_build()
        kwargs.pop('return_factors', None)
        super().build(*args, return_factors=True, **kwargs)
        self.prepare_item_features_transformation()
        self._cold_dev = None
        self._user_factors_device()             # the users' image belongs to the build

    # ---- device state ------------------------------------------------------------------------------------------------
    def _user_factors_device(self):
        """(FactorImage of U diag(sigma) by descending row norm, host int64 order: catalogue position -> training user).
        Belongs to ONE pair of arrays of `factors`: rebuilt after a rank truncation or when a consumer swaps `factors`."""
        U = self.factors.get(self.data.fields.userid, None)
        sigma = self.factors.get('singular_values', None)
        if U is None or sigma is None:
            raise ValueError('%s: no user factors (build the model first)' % self.method)
        cached = self._user_image
        if cached is not None and cached[0] is U and cached[1] is sigma:
            return cached[2], cached[3]
        ops = self.ops
        n_users, rank = U.shape
        if hasattr(ops, 'free_bytes'):
            check_image_memory(n_users, rank, ops.free_bytes())
        kept = self._user_factors_dev
        if (kept is not None and kept[0] is not None and kept[1].shape[0] == n_users and kept[0].strides == U.strides
                and kept[0].__array_interface__['data'][0] == U.__array_interface__['data'][0]):
            Ud = kept[1][:, :rank]              # still on the device from the build (a truncation: its leading columns)
        else:
            Ud = ops.to_device(np.ascontiguousarray(U, dtype=np.float64))
        X = (Ud * ops.to_device(np.asarray(sigma, dtype=np.float64))[None, :]).contiguous()
        order, Xs = self._rows_by_norm(X)
        del X
        image = scoring.FactorImage(ops, Xs)
        self._user_image = (U, sigma, image, order)
        return image, order

    def _features_device(self):
        W = self.item_features_embeddings
        G = self._item_features_transform_helper
        if W is None or G is None:
            raise ValueError('%s: no feature embeddings (build the model first)' % self.method)
        cached = self._features_dev
        if cached is None or cached[0] is not W or cached[1] is not G:
            ops = self.ops
            cached = self._features_dev = (W, G, ops.to_device(np.ascontiguousarray(W, dtype=np.float64)),
                                           ops.to_device(np.ascontiguousarray(G, dtype=np.float64)))
        return cached[2], cached[3]

    def _cold_features_device(self):
        """the one-hot matrix of the cold items over the training labels as a device CSR"""
        key = self.item_features_labels
        if self._cold_dev is None or self._cold_dev[0] is not key:
            F = self._cold_one_hot()
            F.sort_indices()
            if F.shape[1] and F.nnz and (F.indices.min() < 0 or F.indices.max() >= F.shape[1]):
                raise ValueError('cold item features name labels outside the %d training labels' % F.shape[1])
            self._cold_dev = (key, self.ops.csr(F.indptr, F.indices, F.data, F.shape))
        return self._cold_dev[1]

    def _cold_queries_device(self):
        """E = (F_cold W) G on the device, in the layout the candidate sweep reads rows at."""
        F = self._cold_features_device()
        Wd, Gd = self._features_device()
        if F.shape[1] != Wd.shape[0]:
            raise ValueError('cold item features over %d labels, the embeddings over %d' % (F.shape[1], Wd.shape[0]))
        return self.ops.coldstart_queries(F, Wd, Gd)


class SVDModelItemColdStart(ItemColdStartEvaluationMixin, ItemColdStartRecommenderMixin, ItemColdStartSVDModelMixin, SVDModel):
    """coldstart/models.py:225-236."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'PureSVD(cs)'

    def compute_item_features_mapping(self, item_features):
        """W = F_train^T V"""
        V = np.asarray(self.factors[self.data.fields.itemid])
        return np.asarray(item_features.T @ V)


class HybridSVDItemColdStart(ItemColdStartEvaluationMixin, ItemColdStartRecommenderMixin, ItemColdStartSVDModelMixin, HybridSVD):
    """coldstart/models.py:239-251: the features meet the RIGHT projector."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'HybridSVD(cs)'

    def compute_item_features_mapping(self, item_features):
        """W = F_train^T vr"""
        vr = np.asarray(self.get_item_projector()[1])
        return np.asarray(item_features.T @ vr)


class ScaledSVDItemColdStart(ScaledMatrixMixin, SVDModelItemColdStart):
    """coldstart/models.py:254."""


class ScaledHybridSVDItemColdStart(ScaledMatrixMixin, HybridSVDItemColdStart):
    """coldstart/models.py:257."""


class PopularityModelItemColdStart(ItemColdStartEvaluationMixin, RecommenderModel):
    """MP(cs), coldstart/models.py:79-98: the most active training users (of the representative users when there are
    some), the same list for every cold item.  Host only.  Users of equal activity come by ascending id (the reference's
    `sort_values` leaves their order undefined)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.method = 'MP(cs)'
        self.user_scores = None

    def build(self):
        d = self.data
        if _frame_data(d):
            users = np.asarray(d.training[d.fields.userid].values, dtype=np.int64)
        else:
            users = np.asarray(d.training.userid, dtype=np.int64)
        n_users = self._cold_shape()[1]
        activity = np.bincount(users, minlength=n_users)
        ids = self._representative_users()
        if ids is None:
            ids = np.flatnonzero(activity > 0)               # value_counts: the users that occur
        order = np.argsort(-activity[ids], kind='stable')
        self.user_scores = (ids[order], activity[ids][order])   # (user ids, their activity), most active first

    def get_recommendations(self):
        n_cold = self._cold_shape()[0]
        top = np.asarray(self.user_scores[0][:self.topk], dtype=np.int64)
        return np.broadcast_to(top, (n_cold, len(top))).copy()
