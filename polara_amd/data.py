"""ArrayData: the slice of the `RecommenderData` protocol that the factorization-and-scoring hot
path touches, backed by plain NumPy triplets.

It lets the device models run and be benchmarked where Polara itself (pandas state machine,
polara/recommender/data.py) is not installed — e.g. the GPU box.  When Polara is present, the same
model classes accept its `RecommenderData` unchanged, because they only use:
  fields, subscribe/on_change_event/on_update_event, to_coo, test_to_coo, get_test_shape,
  warm_start, test_sample, holdout_size, test.testset/test.holdout.
Semantics restated from data.py:777-884 (threshold_data, to_coo, test_to_coo, get_test_shape).
"""
from collections import namedtuple
from weakref import WeakKeyDictionary
import numpy as np

Fields = namedtuple('Fields', 'userid itemid feedback')
TestData = namedtuple('TestData', 'testset holdout')
Triplets = namedtuple('Triplets', 'userid itemid feedback')


class _Notifier:
    """Weak-reference observer used by RecommenderData (data.py:35-76): callbacks must be bound
    methods; they are invoked as func(subscriber)."""

    def __init__(self, events):
        self._subs = {e: WeakKeyDictionary() for e in events}

    def subscribe(self, event, callback):
        self._subs[event].setdefault(callback.__self__, set()).add(callback.__func__)

    def __call__(self, event):
        for ref in list(self._subs[event].keyrefs()):
            sub = ref()
            if sub is not None:
                for func in list(self._subs[event].get(sub, ())):
                    func(sub)


class ArrayData:
    """training: (users, items, feedback) arrays with contiguous 0-based ids.
    test: triplets of the test users' known interactions, sorted by user (ids are re-based by the
    model exactly like models.py:244-255), or None when test users are training users
    (warm_start=False: the testset is recovered from the training rows of the holdout users,
    data.py:820-832).  holdout: triplets hidden from the model (consumed by evaluation only)."""

    @staticmethod
    def _frozen(u, i, f):
        """The stored columns: arrays that already have the working types are ALIASED, not copied (480 MB at 2e7 entries).
        The contract: the caller does not write to them afterwards — cached level sets, test-user counts and
        device images would go stale with no change event.  The stored views are marked read-only, so a write through
        `data.training` / `data.test` raises; a write through the caller's own reference cannot be caught — call
        `set_training_data` / `set_test_data` with the new arrays instead."""
        out = []
        for a, dt in ((u, np.int64), (i, np.int64), (f, np.float64)):
            a = np.asarray(a)
            v = a.astype(dt, copy=False)
            if v is a or v.base is not None:
                v = v.view()
            v.setflags(write=False)
            out.append(v)
        return Triplets(*out)

    def __init__(self, training, n_users=None, n_items=None, test=None, holdout=None, warm_start=False,
                 fields=('userid', 'itemid', 'rating'), holdout_size=None):
        u, i, f = (np.asarray(a) for a in training)
        self._train = self._frozen(u, i, f)
        self.n_users = int(n_users if n_users is not None else u.max() + 1)
        self.n_items = int(n_items if n_items is not None else i.max() + 1)
        self.fields = Fields(*fields)
        self.warm_start = bool(warm_start)
        self.test_sample = None
        # the reference takes holdout_size from the data configuration (data.py: `holdout_size`), where it always
        # equals the number of items actually held out per user; here it is inferred from the holdout itself
        # (largest number of holdout items of a user) unless given — and a given value must agree with the holdout,
        # because evaluate() switches to the HR / reciprocal-rank family when it is 1 (models.py:453-462)
        self._holdout_size_given = holdout_size
        self.holdout_size = holdout_size if holdout_size is not None else 0
        self.on_change_event = 'on_change'
        self.on_update_event = 'on_update'
        self._notify = _Notifier([self.on_change_event, self.on_update_event])
        self._feedback_levels = None
        self.set_test_data(test, holdout, notify=False)

    # ---- observer protocol (data.py:160-164) ----------------------------------------------------
    def subscribe(self, event, model_callback):
        self._notify.subscribe(event, model_callback)

    def update(self):
        pass

    @property
    def training(self):
        return self._train

    @property
    def test(self):
        return self._test

    def set_training_data(self, training):
        u, i, f = (np.asarray(a) for a in training)
        self._train = self._frozen(u, i, f)
        self._feedback_levels = None
        self._notify(self.on_change_event)

    def set_test_data(self, testset=None, holdout=None, notify=True):
        def norm(t):
            if t is None:
                return None
            u, i, f = (np.asarray(a) for a in t)
            if len(u) < 2 or bool((u[1:] >= u[:-1]).all()):
                # already sorted by user (the usual case): a stable sort would be the identity — no order array, no gathers
                return self._frozen(u, i, f)
            order = np.argsort(u, kind='stable')  # data.py `_try_sort_test_data`
            return Triplets(u[order].astype(np.int64), i[order].astype(np.int64),
                            np.asarray(f, dtype=np.float64)[order])
        self._test = TestData(norm(testset), norm(holdout))
        self._set_holdout_size()
        self._holdout_size_given = None      # the constructor's value described the constructor's holdout only
        if notify:
            self._notify(self.on_update_event)

    def _set_holdout_size(self):
        hold = self._test.holdout
        per_user = 0
        if hold is not None and len(hold.userid):
            u = hold.userid
            first = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])          # sorted by user (set_test_data)
            per_user = int(np.diff(np.r_[first, len(u)]).max())
        given = getattr(self, '_holdout_size_given', None)
        if given is not None and hold is not None and int(given) != per_user:
            raise ValueError('holdout_size=%d, but the holdout has up to %d items per user' % (given, per_user))
        self.holdout_size = int(given) if given is not None else per_user

    # ---- the hot-path protocol ----------------------------------------------------------------------
    @staticmethod
    def threshold_data(idx, val, threshold, filter_values=True):
        """data.py:777-791."""
        if threshold is None:
            return idx, val
        keep = val >= threshold
        if filter_values:
            val = val[keep]
            idx = tuple(x[keep] for x in idx) if isinstance(idx, tuple) else idx[keep, :]
        else:
            val = val.copy()
            val[~keep] = 0
        return idx, val

    def _levels(self):
        if self._feedback_levels is None:
            self._feedback_levels = np.unique(self._train.feedback)  # sorted, like reindex(sort=True)
        return self._feedback_levels

    def to_coo(self, tensor_mode=False, feedback_threshold=None):
        """data.py:794-817."""
        u, i, f = self._train
        if tensor_mode:
            new_f = np.searchsorted(self._levels(), f)
            idx = np.stack([u, i, new_f], axis=1)
            val = np.ones(len(f))
            shp = (self.n_users, self.n_items, len(self._levels()))
        else:
            idx = np.stack([u, i], axis=1)
            val = f
            shp = (self.n_users, self.n_items)
        idx, val = self.threshold_data(idx, val, feedback_threshold)
        return idx.astype(np.intp, copy=False), np.ascontiguousarray(val), tuple(int(s) for s in shp)

    def matrix_triplets(self, feedback_threshold=None):
        """(users, items, feedback, shape) of `to_coo(tensor_mode=False)` WITHOUT the [nnz x 2] index array: the three
        columns as they lie in memory.  A shortcut for device models (the stacked copy of a 2e7-entry index is 35 ms of
        host time next to a 55 ms solver); anything written against the reference's protocol calls `to_coo`."""
        u, i, f = self._train
        (u, i), f = self.threshold_data((u, i), f, feedback_threshold)
        return u, i, np.ascontiguousarray(f), (int(self.n_users), int(self.n_items))

    def tensor_triplets(self):
        """(users, items, feedback, levels, shape) of `to_coo(tensor_mode=True)` WITHOUT the stacked [nnz x 3] index: the
        columns as they lie and the sorted feedback levels, for a device model that looks the level of every entry up (and
        relabels the items) on the device — the stacked index and its host-side passes are a quarter of a 50 ms HOOI
        build.  Anything written against the reference's protocol calls `to_coo`."""
        u, i, f = self._train
        levels = self._levels()
        return u, i, f, levels, (int(self.n_users), int(self.n_items), len(levels))

    def _recover_testset(self):
        """data.py:820-832: training rows of the holdout users, sorted by user."""
        users = np.unique(self._test.holdout.userid)
        u, i, f = self._train
        if len(users) == self.n_users:
            sel = slice(None)
        else:
            sel = np.isin(u, users)
        u, i, f = u[sel], i[sel], f[sel]
        order = np.argsort(u, kind='stable')
        return Triplets(u[order], i[order], f[order])

    def test_to_coo(self, tensor_mode=False, feedback_threshold=None):
        """data.py:835-862."""
        testset = self._test.testset
        if testset is None:
            if self.warm_start or self._test.holdout is None:
                raise ValueError('Unable to read test data')
            testset = self._recover_testset()
        u, i, f = testset
        if tensor_mode:
            levels = self._levels()
            pos = np.searchsorted(levels, f)
            if (pos >= len(levels)).any() or (levels[np.minimum(pos, len(levels) - 1)] != f).any():
                raise NotImplementedError('Not all values of feedback are present in training data')
            coo, val = (u, i), pos.astype(np.intp)
        else:
            coo, val = (u, i), f
        coo, val = self.threshold_data(coo, val, feedback_threshold, filter_values=False)
        return coo + (val,)

    def get_test_shape(self, tensor_mode=False):
        """data.py:865-884."""
        src = self._test.holdout if self._test.holdout is not None else self._test.testset
        if getattr(self, '_n_test_users', None) is None or self._n_test_users[0] is not src:
            u = src.userid                                   # sorted by user (set_test_data): distinct = boundaries + 1
            self._n_test_users = (src, (int(np.count_nonzero(u[1:] != u[:-1])) + 1) if len(u) else 0)
        num_users = self._n_test_users[1]
        shape = (num_users, self.n_items)
        if tensor_mode:
            shape = shape + (len(self._levels()),)
        return shape


class ShardedArrayData(ArrayData):
    """One rank's row block of a user-sharded dataset (polara_amd/shards.py).

    User ids are LOCAL (0 .. hi-lo); `user_range = (lo, hi)` places the block among `n_users_total` users.
    A model built on it with the job's communicator factorizes the WHOLE matrix (item factors, singular values
    and — for CoFFee — feedback factors and core are global and identical on every rank) while everything
    per-user stays with the rank that owns the user: the user-factor rows, `get_recommendations()` and
    `evaluate()` cover the local users only (nothing of size n_users x topk is gathered; sum the hit counts
    over ranks for job-wide metrics).  score_all=True makes every local user a test user with its training
    row as the known preferences; with a `holdout` (local user ids) the test users are the holdout's users and
    their known preferences are recovered from the training rows (the reference's `test_ratio=0,
    warm_start=False` state, data.py:820-832)."""

    def __init__(self, block, n_users_total, feedback_levels=None, score_all=True, holdout=None,
                 fields=('userid', 'itemid', 'rating')):
        indptr = np.asarray(block.indptr, dtype=np.int64)
        u = np.repeat(np.arange(block.n_rows, dtype=np.int64), np.diff(indptr))
        i = np.asarray(block.indices, dtype=np.int64)
        f = np.ones(len(i)) if block.values is None else np.asarray(block.values, dtype=np.float64)
        self.user_range = (int(block.row_lo), int(block.row_hi))
        self.n_users_total = int(n_users_total)
        self.local_csr = block
        self._fixed_levels = None if feedback_levels is None else np.asarray(feedback_levels, dtype=np.float64)
        # the users to score are exactly the training rows: a model may score its device-resident training matrix
        self.scores_training_rows = bool(score_all and holdout is None)
        super().__init__((u, i, f), n_users=block.n_rows, n_items=block.n_cols,
                         test=(u, i, f) if (score_all and holdout is None) else None, holdout=holdout, fields=fields)

    @classmethod
    def from_shards(cls, path, rank=0, world=1, **kwargs):
        """The block of rank `rank` of `world` from a dataset directory written by shards.write_csr_shards /
        ShardWriter."""
        from .shards import load_rank_block
        block, manifest = load_rank_block(path, rank, world)
        kwargs.setdefault('feedback_levels', manifest.get('feedback_levels'))
        return cls(block, manifest['n_rows'], **kwargs)

    def set_test_data(self, testset=None, holdout=None, notify=True):
        if hasattr(self, 'scores_training_rows') and hasattr(self, '_test'):
            self.scores_training_rows = False          # an explicit test set from now on
        super().set_test_data(testset, holdout, notify)

    def set_training_data(self, training):
        raise NotImplementedError('a shard is immutable: write a new dataset (polara_amd.shards) instead')

    def _levels(self):
        # the SAME level set on every rank (a block need not contain every level)
        if self._fixed_levels is not None:
            return self._fixed_levels
        return super()._levels()


class SimilarityArrayData(ArrayData):
    """ArrayData with side relations: the counterpart of Polara's `SimilarityDataModel` (SideRelationsMixin +
    IdentityDiagonalMixin, hybrid/data.py:8-69) for HybridSVD.

    relations_matrices: {entity field name: square SciPy sparse matrix or ndarray, or None}; relations_indices: {entity
    field name: the entity id of every row of that matrix, or None when row r IS entity r}.  `get_relations_matrix(entity)`
    returns the matrix in the data's id order with its diagonal set to 1 (a copy: the caller's matrix is not written), built
    on first use and dropped on a data-change event."""

    def __init__(self, training, *args, relations_matrices, relations_indices, **kwargs):
        super().__init__(training, *args, **kwargs)
        self._init_relations(relations_matrices, relations_indices)

    def _init_relations(self, relations_matrices, relations_indices):
        entities = (self.fields.userid, self.fields.itemid)
        self._rel_mat = {e: m for e, m in relations_matrices.items() if e in entities}
        self._rel_idx = {e: (None if idx is None else np.asarray(idx)) for e, idx in relations_indices.items() if e in entities}
        self._relations = dict.fromkeys(entities)
        self.subscribe(self.on_change_event, self._clean_relations)

    def _clean_relations(self):
        self._relations = dict.fromkeys(self._relations.keys())

    @property
    def item_relations(self):
        return self.get_relations_matrix(self.fields.itemid)

    @property
    def user_relations(self):
        return self.get_relations_matrix(self.fields.userid)

    def get_relations_matrix(self, entity):
        if self._relations.get(entity, None) is None:
            self._update_relations(entity)
        return self._relations[entity]

    def _update_relations(self, entity):
        from scipy.sparse import issparse
        mat = self._rel_mat.get(entity, None)
        if mat is None:
            self._relations[entity] = None
            return
        n = self.n_users if entity == self.fields.userid else self.n_items
        idx = self._rel_idx.get(entity, None)
        if idx is None:
            if mat.shape[0] != n:
                raise ValueError('%s relations: %d rows for %d entities' % (entity, mat.shape[0], n))
            rows = np.arange(n)
        else:
            pos = {int(e): p for p, e in enumerate(idx)}          # entity id -> row of the relations matrix
            missing = [e for e in range(n) if e not in pos]
            if missing:
                raise ValueError('%s relations: no row for %d entities (first: %d)' % (entity, len(missing), missing[0]))
            rows = np.fromiter((pos[e] for e in range(n)), dtype=np.int64, count=n)
        if issparse(mat):
            rel = mat.tocsr()[:, rows][rows, :].tocsr()
            rel.setdiag(1)
        else:
            rel = np.array(np.asarray(mat)[np.ix_(rows, rows)], dtype=np.float64)
            np.fill_diagonal(rel, 1)
        self._relations[entity] = rel


class ItemPostFilteringArrayData(ArrayData):
    """ArrayData with item contexts: the counterpart of Polara's `ItemPostFilteringData` (contextual/data.py:4-64) for
    `ItemPostFilteringMixin` — every test user comes with one value per context (the value of its held-out interaction: a
    genre, a daypart), every value with a list of items, and the model ranks those items first.

    item_context_mapping: {context: (item_ids, context_values)} — the many-to-many pairs of the reference's mapping frame, in
    the data's item ids; items outside 0..n_items-1 are dropped, repeated pairs count once.  holdout_context: {context: values
    aligned with the holdout rows as given}.  Like the reference (contextual/data.py:42-49) the holdout must have exactly one
    row per user (ValueError otherwise).  A holdout value without items in the mapping gives an empty list (the reference's
    `reindex(..., fill_value=[])`).  The mapped state is recomputed by `set_test_data` (pass the new holdout's
    `holdout_context`) and dropped by a data-change event; it is rebuilt on the next access."""

    def __init__(self, *args, item_context_mapping, holdout_context, **kwargs):
        self._context_mapping = {c: (np.asarray(i, dtype=np.int64), np.asarray(v)) for c, (i, v) in dict(item_context_mapping).items()}
        for c, (i, v) in self._context_mapping.items():
            if i.ndim != 1 or i.shape != v.shape:
                raise ValueError('context %r: %s item ids for %s values' % (c, i.shape, v.shape))
        self._holdout_context_given = dict(holdout_context)
        self._holdout_context = None
        self._context = None
        super().__init__(*args, **kwargs)
        self.subscribe(self.on_change_event, self._clean_context)

    @property
    def contexts(self):
        """the contexts in mapping order: position j is bit j of an item's class"""
        return tuple(self._context_mapping)

    def _clean_context(self):
        self._context = None

    def set_test_data(self, testset=None, holdout=None, notify=True, holdout_context=None):
        if holdout_context is not None:
            self._holdout_context_given = dict(holdout_context)
        self._context = self._holdout_context = None
        if holdout is not None:
            u = np.asarray(holdout[0])
            missing = [c for c in self._context_mapping if c not in self._holdout_context_given]
            if missing:
                raise ValueError('no holdout values for context %r' % (missing[0],))
            cols = {c: np.asarray(self._holdout_context_given[c]) for c in self._context_mapping}
            for c, v in cols.items():
                if v.shape != u.shape:
                    raise ValueError('context %r: %d values for %d holdout rows' % (c, len(v), len(u)))
            if len(u) > 1 and not bool((u[1:] >= u[:-1]).all()):
                order = np.argsort(u, kind='stable')          # the rows are stored sorted by user: the values move with them
                cols = {c: v[order] for c, v in cols.items()}
            self._holdout_context = cols
        super().set_test_data(testset, holdout, notify=False)
        self.update_contextual_data()
        if notify:
            self._notify(self.on_update_event)

    def update_contextual_data(self):
        """contextual/data.py:42-49 with map_context_data (:15-40): per context the sorted distinct values that have items,
        the CSR of their sorted distinct items, and the position of every test user's value among them (-1: no items)."""
        self._context = None
        hold = self._test.holdout
        if hold is None:
            return
        u = hold.userid
        if len(u) > 1 and bool((u[1:] == u[:-1]).any()):
            raise ValueError('contextual post-filtering needs exactly one holdout row per user: %d rows for %d users'
                             % (len(u), int(np.count_nonzero(u[1:] != u[:-1])) + 1))
        mapped = {}
        for c, (items, values) in self._context_mapping.items():
            keep = (items >= 0) & (items < self.n_items)
            vals, inv = np.unique(values[keep], return_inverse=True)
            pairs = np.unique(inv.astype(np.int64).ravel() * self.n_items + items[keep])      # sorted by (value, item), distinct
            value_ptr = np.zeros(len(vals) + 1, dtype=np.int64)
            np.cumsum(np.bincount(pairs // self.n_items, minlength=len(vals)), out=value_ptr[1:])
            hv = self._holdout_context[c]
            user_value = np.full(len(u), -1, dtype=np.int32)
            if len(vals) and len(hv):
                try:
                    pos = np.minimum(np.searchsorted(vals, hv), len(vals) - 1)
                    hit = vals[pos] == hv
                except TypeError:                                    # values of another kind than the mapping's: none matches
                    pos, hit = np.zeros(len(hv), dtype=np.int64), np.zeros(len(hv), dtype=bool)
                user_value[hit] = pos[hit]
            mapped[c] = (vals, value_ptr, (pairs % self.n_items).astype(np.int64), user_value)
        self._context = mapped

    def _mapped(self, context):
        if self._context is None:
            self.update_contextual_data()
        if self._context is None:
            raise ValueError('no holdout: the contexts have nothing to map')
        return self._context[context]

    @property
    def context_data(self):
        """{context: (values, value_ptr, value_items, user_value)} in mapping order: the mapped state as one object, replaced
        whenever it is recomputed (what a model keys its device images by)"""
        if self._context is None:
            self.update_contextual_data()
        return self._context

    def context_values(self, context):
        """(sorted distinct values, value_ptr int64 [n_values + 1], value_items int64 in the data's item ids, sorted and
        distinct per value)"""
        return self._mapped(context)[:3]

    def user_context(self, context):
        """int32 per test user (the distinct holdout users, sorted): the position of its value in `context_values`, -1 when
        the value has no items"""
        return self._mapped(context)[3]


def one_hot_csr(features, n_rows=None, n_labels=None):
    """A SciPy CSR feature matrix [n_rows x n_labels] from a SciPy matrix or from one list of label ids per row (the
    layout `stack_features(..., normalize=False)` gives the reference, lib/similarity.py:327-348): canonical (sorted
    indices, duplicates summed), fp64."""
    from scipy.sparse import csr_matrix, issparse
    if issparse(features):
        m = csr_matrix(features, dtype=np.float64)
    else:
        rows = [np.unique(np.asarray(r, dtype=np.int64)) for r in features]      # a label counts once (feature2sparse: set)
        indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
        indices = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        width = int(n_labels if n_labels is not None else (indices.max() + 1 if len(indices) else 0))
        if len(indices) and (indices.min() < 0 or indices.max() >= width):      # (SciPy's constructor does not check this)
            raise ValueError('feature label %d outside the %d labels' % (int(indices.max() if indices.min() >= 0 else indices.min()), width))
        m = csr_matrix((np.ones(len(indices)), indices, indptr), shape=(len(rows), width))
    if n_rows is not None and m.shape[0] != n_rows:
        raise ValueError('features for %d rows, %d expected' % (m.shape[0], n_rows))
    if n_labels is not None and m.shape[1] != n_labels:
        raise ValueError('features over %d labels, %d expected' % (m.shape[1], n_labels))
    m.sum_duplicates()
    m.sort_indices()
    return m


class ItemColdStartArrayData(ArrayData):
    """ArrayData for item cold start: the counterpart of Polara's `ItemColdStartData` (coldstart/data.py:10-225) after
    `prepare()`.

    training: triplets of the training (warm) items, as in ArrayData.  holdout: triplets (user, cold item, feedback) with the
    cold items numbered 0..n_cold-1; kept sorted by cold item (coldstart/data.py:212-217).  item_features /
    cold_item_features: the features of the training items (rows in item id order) and of the cold items over ONE label
    space — SciPy matrices, or one list of label ids per item.  Cold items that share no label with any training item are
    dropped and the remaining ones renumbered, in the feature matrix and in the holdout (`is_valid`,
    coldstart/data.py:162-209); `cold_items_kept` holds their original numbers.  representative_users: sorted internal user
    ids or None (`data.representative_users`; only MP(cs) restricts itself to them).  `holdout_size` reads -1."""

    def __init__(self, training, holdout, item_features, cold_item_features, n_users=None, n_items=None,
                 representative_users=None, fields=('userid', 'itemid', 'rating')):
        self._constructing = True               # the base constructor sets an empty test state through set_test_data
        ArrayData.__init__(self, training, n_users=n_users, n_items=n_items, fields=fields)
        self._constructing = False
        self.item_features = one_hot_csr(item_features, n_rows=self.n_items)
        self._set_cold_items(holdout, cold_item_features)
        self.representative_users = (None if representative_users is None
                                     else np.unique(np.asarray(representative_users, dtype=np.int64)))
        if self.representative_users is not None and len(self.representative_users) and not (
                0 <= self.representative_users[0] and self.representative_users[-1] < self.n_users):
            raise ValueError('representative users outside 0..%d' % (self.n_users - 1))

    @property
    def holdout_size(self):
        return -1

    @holdout_size.setter
    def holdout_size(self, new_value):
        if new_value:                       # (0 is what the base constructor writes; coldstart/data.py:30-35)
            raise NotImplementedError('Setting holdout size is currently not supported in item cold start.')

    def _set_holdout_size(self):
        pass

    def _set_cold_items(self, holdout, cold_item_features):
        cold = one_hot_csr(cold_item_features, n_labels=self.item_features.shape[1])
        known = np.diff(self.item_features.tocsc().indptr) > 0                 # labels some training item carries
        valid = np.asarray(cold[:, np.flatnonzero(known)].getnnz(axis=1)).ravel() > 0
        u, c, f = (np.asarray(a) for a in holdout)
        c = c.astype(np.int64)
        if len(c) and (c.min() < 0 or c.max() >= cold.shape[0]):
            raise ValueError('holdout names cold item %d, the features describe %d cold items' % (int(c.max()), cold.shape[0]))
        if len(u) and (u.min() < 0 or u.max() >= self.n_users):
            raise ValueError('holdout names user %d of %d training users' % (int(u.max()), self.n_users))
        self.cold_items_kept = np.flatnonzero(valid)
        new_id = np.full(cold.shape[0], -1, dtype=np.int64)
        new_id[self.cold_items_kept] = np.arange(len(self.cold_items_kept))
        keep = valid[c]
        u, c, f = u[keep], new_id[c[keep]], np.asarray(f, dtype=np.float64)[keep]
        order = np.argsort(c, kind='stable')
        self.cold_item_features = cold[self.cold_items_kept]
        self.n_cold_items = int(len(self.cold_items_kept))
        self._test = TestData(None, self._frozen(u[order], c[order], f[order]))

    def set_test_data(self, testset=None, holdout=None, notify=True, cold_item_features=None):
        """A new holdout (user, cold item, feedback), with the features of its cold items when those change too."""
        if self._constructing:
            self._test = TestData(None, None)       # (the holdout follows once the features are known)
            return
        if holdout is None:
            raise ValueError('item cold start needs a holdout of (user, cold item, feedback) triplets')
        self._set_cold_items(holdout, self.cold_item_features if cold_item_features is None else cold_item_features)
        if notify:
            self._notify(self.on_update_event)

    def get_test_shape(self, tensor_mode=False):
        """(cold items, training items): the models take (n_cold_items, n_users) from the data instead."""
        shape = (self.n_cold_items, self.n_items)
        return shape + (len(self._levels()),) if tensor_mode else shape


class ItemColdStartSimilarityArrayData(ItemColdStartArrayData, SimilarityArrayData):
    """ItemColdStartArrayData plus the relations of SimilarityArrayData (the counterpart of `ItemColdStartSimilarityData`,
    coldstart/data.py:256-259) — what the hybrid cold-start models are built on.

    cold_relations_matrices (optional): {item field name: M}, M the similarity of the cold items, as numbered in the
    holdout, to the training items [cold items x n_items], a SciPy sparse matrix or an ndarray — what SIM(cs) aggregates
    over (`cold_items_similarity`, coldstart/data.py:228-253)."""

    def __init__(self, training, holdout, item_features, cold_item_features, *, relations_matrices, relations_indices,
                 cold_relations_matrices=None, **kwargs):
        self._cold_rel_mat = dict(cold_relations_matrices or {})
        self._cold_similarity = None
        ItemColdStartArrayData.__init__(self, training, holdout, item_features, cold_item_features, **kwargs)
        self._init_relations(relations_matrices, relations_indices)

    def _set_cold_items(self, holdout, cold_item_features):
        super()._set_cold_items(holdout, cold_item_features)
        self._cold_similarity = None                # the cold items that survive the validity filter may have changed

    @property
    def cold_items_similarity(self):
        """fp64 SciPy CSR [n_cold_items x n_items]: the rows `cold_items_kept` of the given matrix, in the cold items' new
        numbering, no diagonal treatment (the reference's `sim_mat[:, seen_idx][cold_idx, :]`); None when no cold relations
        were given.  The entries of a row keep the order in which the given matrix stores them — the reference's matrix comes
        out of its indexing unsorted, SIM(cs) adds a row's products in the stored order, and another order changes the last
        bits of a score."""
        mat = self._cold_rel_mat.get(self.fields.itemid, None)
        if mat is None:
            return None
        if self._cold_similarity is None:
            from scipy.sparse import csr_matrix
            m = csr_matrix(mat, dtype=np.float64)
            if m.shape[1] != self.n_items or (len(self.cold_items_kept) and self.cold_items_kept[-1] >= m.shape[0]):
                raise ValueError('cold item relations of shape %s: %d training items and cold items up to number %d expected'
                                 % (m.shape, self.n_items, int(self.cold_items_kept[-1]) if len(self.cold_items_kept) else -1))
            self._cold_similarity = m[self.cold_items_kept]
        return self._cold_similarity


class RandomSampleEvaluationMixin:
    """The data side of the sampled-negatives protocol (the reference's `RandomSampleEvaluationMixin`, data.py:938-994) on
    arrays: every holdout item of a test user is ranked against a fixed number of items the user has not seen, given
    explicitly (`set_unseen_interactions`) or drawn by the model (`unseen_items_num` and `seed`).

    unseen_interactions: int64 [n_test_users x n] of internal item ids, row r for the r-th test user in sorted order, or
    None.  unseen_items_num: n, or None.  `adapt_holdout()` gives the column of every holdout entry in the model's score
    rows `[holdout items | unseen items]` — the reference's `cumcount`, kept in `holdout_positions`.

    One difference from the reference: new test data (`set_test_data`) clears `unseen_interactions` — the stored rows
    belong to the former test users; the reference keeps them and fails or mis-scores at the next lookup."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.unseen_interactions = None
        self.unseen_items_num = None
        self._holdout_item_prefix = 'x'
        self.holdout_positions = None
        if not hasattr(self, 'seed'):
            self.seed = None

    def set_test_data(self, *args, **kwargs):
        super().set_test_data(*args, **kwargs)
        self.unseen_interactions = None
        self.holdout_positions = None

    def adapt_holdout(self):
        """int64 [n_holdout]: the position of every holdout entry among its user's entries (0, 1, ...) in the order of the
        stored holdout, which is sorted by user."""
        hold = self.test.holdout
        if hold is None:
            raise ValueError('adapt_holdout() needs a holdout')
        u = np.asarray(hold.userid)
        first = np.flatnonzero(np.r_[True, u[1:] != u[:-1]]) if len(u) else np.zeros(0, dtype=np.int64)
        start = np.repeat(first, np.diff(np.r_[first, len(u)]))
        self.holdout_positions = (np.arange(len(u)) - start).astype(np.int64)
        return self.holdout_positions

    def set_unseen_interactions(self, interactions, reindex=False):
        """`interactions`: [n_test_users x n] internal item ids (any integer type; a list of equally long lists will do)."""
        if reindex:
            raise NotImplementedError('arrays carry internal ids only: reindex=True has nothing to map')
        try:
            arr = np.asarray(interactions)
        except ValueError:                                     # NumPy >= 1.24 refuses a ragged list
            arr = np.empty(0, dtype=object)
        n_test_users = int(self.get_test_shape(tensor_mode=False)[0])
        if arr.dtype == object or arr.ndim != 2:
            raise ValueError('Number of unseen items is inconsistent')
        if arr.shape[0] != n_test_users or arr.shape[1] < 1:
            raise ValueError('unseen interactions of shape %s for %d test users' % (arr.shape, n_test_users))
        if not np.issubdtype(arr.dtype, np.integer):
            raise ValueError('unseen interactions must hold integer item ids, got %s' % arr.dtype)
        if arr.min() < 0 or arr.max() >= self.n_items:
            raise ValueError('unseen interactions name item %d of %d' % (int(arr.max() if arr.min() >= 0 else arr.min()), self.n_items))
        self.unseen_interactions = np.ascontiguousarray(arr, dtype=np.int64)
        self.unseen_items_num = int(arr.shape[1])
        self.adapt_holdout()


class RandomSampleArrayData(RandomSampleEvaluationMixin, ArrayData):
    """ArrayData for the sampled-negatives protocol; `seed` feeds the per-user seeds of the model's sampler
    (`np.random.SeedSequence(seed).generate_state(n_test_users)`, models.py:1151)."""

    def __init__(self, *args, seed=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.seed = seed
