"""Sampled-negatives evaluation on the device: the reference's `RandomSampleEvaluationSVDMixin` (models.py:1095-1183).

Every holdout item of a test user is ranked against a fixed number of items the user has not seen — the protocol of the
PureSVD paper (1 holdout item + 1000 unseen ones).  The score row of a user is `[holdout items | unseen items]`, the lists
hold COLUMN POSITIONS of that row, and a holdout item is "hit" when its own position (0 .. holdout_size-1) is in the list.
Three device calls: the fold-in P = T V (the fp64 SpMM every model uses), optionally the sampler (pk_sample_unseen) and one
gathered product with the top-k fused in (pk_candidates_topk_f64), whose sums run in the order of the reference's
`inner_product_at` without contraction.

The first part is host-side checking, pure Python (tests/test_sampled_host.py)."""
import numpy as np

from .models import ScaledSVD, SVDModel


def check_candidate_shapes(p_shape, v_shape, cand_shape, topk):
    """(n_users, r, n_items, C) of a candidate pass; the ranges of r and topk are the library's to check."""
    if len(p_shape) != 2 or len(v_shape) != 2 or len(cand_shape) != 2:
        raise ValueError('candidates_topk: P %s, V %s and the candidates %s must be matrices'
                         % (tuple(p_shape), tuple(v_shape), tuple(cand_shape)))
    n_users, r = (int(x) for x in p_shape)
    n_items, rv = (int(x) for x in v_shape)
    if rv != r:
        raise ValueError('candidates_topk: user factors of rank %d, item factors of rank %d' % (r, rv))
    if int(cand_shape[0]) != n_users:
        raise ValueError('candidates_topk: candidates for %d users, factors of %d' % (int(cand_shape[0]), n_users))
    return n_users, r, n_items, int(cand_shape[1])


def check_sample_request(n, n_items, n_seeds, n_users, max_n):
    if n < 1 or n > max_n:
        raise ValueError('sample_unseen: %d items per user outside 1..%d' % (n, max_n))
    if n > n_items:
        raise ValueError('sample_unseen: %d items per user from a catalogue of %d' % (n, n_items))
    if n_seeds != n_users:
        raise ValueError('sample_unseen: %d seeds for %d users' % (n_seeds, n_users))


def fewest_eligible_items(t_indptr, t_indices, h_indptr, h_indices, n_items):
    """The smallest number of items outside the union of its two rows that any user has."""
    return int(n_items - _excluded_counts(t_indptr, t_indices, h_indptr, h_indices, n_items).max())


def users_short_of_items(t_indptr, t_indices, h_indptr, h_indices, n_items, n):
    """The users with fewer than n items outside the union of their two rows (the reference would fail in `randrange(0)`)."""
    return np.flatnonzero(n_items - _excluded_counts(t_indptr, t_indices, h_indptr, h_indices, n_items) < n)


def _excluded_counts(t_indptr, t_indices, h_indptr, h_indices, n_items):
    t_indptr = np.asarray(t_indptr, dtype=np.int64)
    excluded = np.diff(t_indptr)
    if h_indptr is not None:
        h_indptr = np.asarray(h_indptr, dtype=np.int64)
        n_users = len(t_indptr) - 1
        t_keys = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(t_indptr)) * n_items + np.asarray(t_indices[:t_indptr[-1]], dtype=np.int64)
        h_rows = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(h_indptr))
        h_keys = np.unique(h_rows * n_items + np.asarray(h_indices[:h_indptr[-1]], dtype=np.int64))
        new = h_keys[~np.isin(h_keys, t_keys)]
        excluded = excluded + np.bincount(new // n_items, minlength=n_users)
    return excluded


def user_seeds(seed, n_users):
    """One uint32 per user: the reference's line (models.py:1151)."""
    return np.random.SeedSequence(seed).generate_state(int(n_users))


class RandomSampleEvaluationSVDMixin:
    """Mix into a factorization model (before it): `get_recommendations` then ranks `[holdout | unseen]` per test user and
    returns column positions.  The unseen items are `data.unseen_interactions`, or — when only `data.unseen_items_num` is
    set — drawn per user from the items outside its test row and its holdout with seeds from `data.seed`.  The sampled
    stream is this package's own.  `filter_seen` plays no part.  Setting `_prediction_target` back to
    the item field restores the parent's full-catalogue lists (models.py:1160-1161)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        prefix = getattr(self.data, '_holdout_item_prefix', 'x')
        self._prediction_target = '%s_%s' % (prefix, self.data.fields.itemid)

    # ---- what the data object holds, pandas or arrays ------------------------------------------------------------
    def _sampled_single_process(self):
        if self.comm.world > 1:
            raise NotImplementedError('%s: sampled evaluation runs in one process (comm.world = %d)'
                                      % (self.method, self.comm.world))

    def _holdout_columns(self):
        hold = self.data.test.holdout
        if hold is None:
            raise ValueError('sampled evaluation needs a holdout')
        if hasattr(hold, 'columns'):                       # Polara's data model: a frame sorted by user
            f = self.data.fields
            return np.asarray(hold[f.userid].values), np.asarray(hold[f.itemid].values, dtype=np.int64)
        return np.asarray(hold.userid), np.asarray(hold.itemid, dtype=np.int64)

    def _holdout_items(self):
        """int64 [n_holdout_users x holdout_size]: the holdout items of every test user in holdout order (sorted by user)."""
        h = self.data.holdout_size
        if h is None or int(h) < 1:
            raise ValueError('sampled evaluation needs a fixed holdout_size >= 1, got %r' % (h,))
        h = int(h)
        users, items = self._holdout_columns()
        if len(users) == 0 or len(users) % h:
            raise ValueError('a holdout of %d entries is not %d per user' % (len(users), h))
        by_user = users.reshape(-1, h)
        if (by_user != by_user[:, :1]).any() or (np.diff(by_user[:, 0]) <= 0).any():
            raise ValueError('every user must have exactly %d holdout items, stored together and sorted by user' % h)
        return np.ascontiguousarray(items.reshape(-1, h))

    def _stored_unseen(self, n_users):
        """int64 [n_users x n] from `data.unseen_interactions` (an array, or the reference's Series of arrays), or None."""
        ui = getattr(self.data, 'unseen_interactions', None)
        if ui is None:
            return None
        if hasattr(ui, 'loc'):
            users = self._holdout_columns()[0]
            test_users = users[np.r_[True, users[1:] != users[:-1]]]
            ui = np.stack([np.asarray(x) for x in ui.loc[test_users].values])
        ui = np.asarray(ui, dtype=np.int64)
        if ui.ndim != 2 or ui.shape[0] != n_users:
            raise ValueError('unseen interactions of shape %s for %d test users' % (ui.shape, n_users))
        return ui

    def _internal(self, items):
        """device int32 of item ids in the model's internal order"""
        ops = self.ops
        if torch_is_tensor(items):
            t = items.long()
        else:
            t = ops.to_device(np.ascontiguousarray(items, dtype=np.int64))
        if self._item_rank is not None:
            cached = getattr(self, '_rank_dev', None)
            if cached is None or cached[0] is not self._item_rank:      # one upload per item order
                cached = self._rank_dev = (self._item_rank, ops.to_device(np.ascontiguousarray(self._item_rank, dtype=np.int64)))
            t = cached[1][t]
        return t.int()

    def _test_csr_in_data_ids(self, T):
        """The device test CSR with the data's item ids as columns (sorted), kept next to the CSR it was made from."""
        if self._item_rank is None:
            return T
        cached = getattr(self, '_test_ext', None)
        if cached is None or cached[0] is not T or cached[1] is not self._item_inv:
            cached = self._test_ext = (T, self._item_inv, self.ops.csr_relabel_cols(T, self._item_inv))
        return cached[2]

    def _sample(self, T_ext, hold_items, n_unseen):
        """device int32 [n_users x n_unseen] in the DATA's item ids: excluded are the user's test row and its holdout."""
        ops = self.ops
        n_users, n_items = T_ext.shape
        rows = np.repeat(np.arange(n_users, dtype=np.int64), hold_items.shape[1])
        H = ops.csr_from_coo(rows, hold_items.reshape(-1), np.ones(hold_items.size), (n_users, n_items))
        return ops.sample_unseen(T_ext, H, int(n_unseen), user_seeds(getattr(self.data, 'seed', None), n_users))

    # ---- the protocol ------------------------------------------------------------------------------------------------
    def sampled_candidates(self):
        """(P, V, cand): the folded-in user factors, the item factors in internal order and the int32 candidates
        `[holdout | unseen]` in internal ids, all on the device."""
        ops = self.ops
        T, n_users, n_items = self._device_test_csr()
        hold_items = self._holdout_items()
        if hold_items.shape[0] != n_users:
            raise ValueError('the holdout names %d users, the test data %d' % (hold_items.shape[0], n_users))
        if hold_items.min() < 0 or hold_items.max() >= n_items:
            raise ValueError('holdout item ids outside 0..%d' % (n_items - 1))
        fac = self._item_factors_device()
        P = ops.spmm(T, fac.fold_in)
        unseen = self._stored_unseen(n_users)
        if unseen is None:
            n_unseen = getattr(self.data, 'unseen_items_num', None)
            if n_unseen is None:
                raise ValueError('Number of items to sample is unspecified.')
            unseen = self._sample(self._test_csr_in_data_ids(T), hold_items, n_unseen)
        elif unseen.size and (unseen.min() < 0 or unseen.max() >= n_items):
            raise ValueError('unseen item ids outside 0..%d' % (n_items - 1))
        import torch
        cand = torch.cat([self._internal(hold_items), self._internal(unseen)], dim=1).contiguous()
        return P, fac.V, cand

    def get_recommendations(self):
        if self._prediction_target == self.data.fields.itemid:
            return super().get_recommendations()
        self._sampled_single_process()
        if self.verify_integrity:
            self.verify_data_integrity()
        P, V, cand = self._checked_candidates()
        recs, _ = self.ops.candidates_topk(P, V, cand, self.topk)
        self._recs_dev = None
        return self.ops.to_host(recs)

    def _checked_candidates(self):
        P, V, cand = self.sampled_candidates()
        if not 1 <= int(self.topk) <= cand.shape[1]:
            raise ValueError('topk = %d with %d candidates per user' % (self.topk, cand.shape[1]))
        return P, V, cand

    def recommend_with_scores(self):
        """(lists of column positions, the fp64 score rows `[holdout | unseen]`, the candidates in the data's item ids):
        host arrays."""
        if not self._is_ready:
            self.build()
        if self._prediction_target == self.data.fields.itemid:
            raise ValueError('recommend_with_scores: the prediction target is the item field — the lists are the parent\'s '
                             'full-catalogue ones (get_recommendations)')
        self._sampled_single_process()
        ops = self.ops
        P, V, cand = self._checked_candidates()
        recs, scores = ops.candidates_topk(P, V, cand, self.topk, want_scores=True)
        items = ops.to_host(cand).astype(np.int64)
        if self._item_inv is not None:
            items = np.asarray(self._item_inv, dtype=np.int64)[items]
        return ops.to_host(recs), ops.to_host(scores), items

    # ---- the reference's three score functions: host arrays in, host arrays out --------------------------------------
    def _scores_at(self, user_factors, item_factors, items):
        ops = self.ops
        P = ops.to_device(np.ascontiguousarray(user_factors, dtype=np.float64))
        V = ops.to_device(np.ascontiguousarray(item_factors, dtype=np.float64))
        cand = items if torch_is_tensor(items) else ops.to_device(np.ascontiguousarray(items, dtype=np.int64))
        return ops.to_host(ops.candidates_topk(P, V, cand.int(), 1, want_scores=True)[1])

    def compute_holdout_scores(self, user_factors, item_factors):
        """fp64 [n_users x holdout_size]: row u of `user_factors` against the holdout items of the u-th test user."""
        return self._scores_at(user_factors, item_factors, self._holdout_items())

    def compute_random_item_scores(self, user_factors, item_factors):
        """fp64 [n_users x n]: against the stored unseen items."""
        unseen = self._stored_unseen(np.asarray(user_factors).shape[0])
        if unseen is None:
            raise ValueError('the data model holds no unseen interactions')
        return self._scores_at(user_factors, item_factors, unseen)

    def compute_random_item_scores_gen(self, user_factors, item_factors, profile_matrix, n_unseen):
        """fp64 [n_users x n_unseen]: against items drawn outside the rows of `profile_matrix` (a SciPy matrix over the
        data's item ids) and the holdout."""
        from scipy.sparse import csr_matrix
        m = csr_matrix(profile_matrix)
        m.sort_indices()
        T_ext = self.ops.csr(m.indptr, m.indices, np.ones(m.nnz), m.shape)
        hold_items = self._holdout_items()
        if hold_items.shape[0] != m.shape[0]:
            raise ValueError('the holdout names %d users, the profile matrix %d' % (hold_items.shape[0], m.shape[0]))
        return self._scores_at(user_factors, item_factors, self._sample(T_ext, hold_items, n_unseen))

    # ---- evaluation ------------------------------------------------------------------------------------------------
    def evaluate(self, metric_type='all', topk=None, not_rated_penalty=None, switch_positive=None,
                 ignore_feedback=False, simple_rates=False, on_feedback_level=None):
        """The parent's `evaluate` with the holdout POSITIONS as targets and the number of candidates as the number of
        entities.  'experience' and 'all' raise ValueError: coverage of column positions means nothing (the reference
        fails at the same place, `fields.index('x_itemid')`, models.py:469)."""
        holdout = self.data.test.holdout
        if self._prediction_target == self.data.fields.itemid or hasattr(holdout, 'columns'):
            return super().evaluate(metric_type=metric_type, topk=topk, not_rated_penalty=not_rated_penalty,
                                    switch_positive=switch_positive, ignore_feedback=ignore_feedback,
                                    simple_rates=simple_rates, on_feedback_level=on_feedback_level)
        from . import evaluation
        wanted = metric_type if isinstance(metric_type, (list, tuple)) else [metric_type]
        if 'all' in wanted or 'experience' in wanted:
            raise ValueError("metric_type %r: '%s' is not in the fields of the data — experience metrics are undefined for "
                             "column positions" % (metric_type, self._prediction_target))
        if holdout is None:
            raise ValueError('evaluate() needs a holdout')
        if int(topk or 0) > self.topk:
            self.topk = topk
        recs = self.recommendations[:, :topk]
        users, _, fdbk = holdout
        users = np.asarray(users)
        positions = getattr(self.data, 'holdout_positions', None)              # the reference's cumcount (data mixin)
        if positions is None or len(positions) != len(users):
            positions = self.data.adapt_holdout()
        n_cand = int(self.data.holdout_size) + int(self.data.unseen_items_num)
        fb = None if fdbk is None else np.asarray(fdbk, dtype=np.float64)
        return evaluation.evaluate(recs, users, np.asarray(positions, dtype=np.int64), fb, n_cand, metric_type=metric_type,
                                   not_rated_penalty=not_rated_penalty,
                                   switch_positive=switch_positive or self.switch_positive,
                                   ignore_feedback=ignore_feedback, simple_rates=simple_rates,
                                   holdout_size=self.data.holdout_size,
                                   ndcg_alternative=_ndcg_alternative())


def torch_is_tensor(x):
    import torch
    return torch.is_tensor(x)


def _ndcg_alternative():
    from .models import get_default
    return get_default('ndcg_alternative')


class SVDModelSampled(RandomSampleEvaluationSVDMixin, SVDModel):
    """PureSVD under the sampled-negatives protocol."""


class ScaledSVDSampled(RandomSampleEvaluationSVDMixin, ScaledSVD):
    """Scaled PureSVD under the sampled-negatives protocol."""
