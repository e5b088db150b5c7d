"""Contextual post-filtering: the counterpart of the reference's `ItemPostFilteringMixin` (contextual/models.py:5-32) over
`ItemPostFilteringArrayData`.

The reference up-votes, on the dense score chunk and context by context, the items in the list of every test user's
context value: s <- M + s + 1 with M the maximum of the chunk.  When every score of the chunk is > -1 that is a
class-lexicographic order — class = sum_j 2^j [item in the list of the user's value of context j], then score, then item —
and it does not depend on the chunking; for scores <= -1 the literal arithmetic is an artefact of the chunk's maximum.

`get_recommendations` serves that ORDER without a dense chunk: the scoring pass gives the class-0 lists as always and
pk_context_merge_f64 (csrc/context.hip) puts the exact tier of the context items on top, from the same query rows E (so a
(user, item) score has the same bits in both).  Seen items are never up-voted: when a row runs out of unseen items its seen
tail follows in the order of the plain pass (the reference would put seen context items first inside that tail).

`slice_recommendations` keeps the reference's protocol for dense consumers (`_user_scores`, `show_recommendations`): the
LITERAL arithmetic, in place on the returned host block, M over the block."""
from collections import namedtuple

import numpy as np

# the device image of one context (ops.context_lists): int32 [n_rows], int64 [n_values + 1], int32 serving positions, int
ContextLists = namedtuple('ContextLists', 'user_value value_ptr value_items max_list')


def check_context_lists(user_value, value_ptr, value_items, n_users, n_items):
    """The host arrays of one context in the types the kernel reads, range-checked (the kernel trusts them):
    (user_value int32, value_ptr int64, value_items int32 — never empty, so that it has an address —, longest list)."""
    uv = np.ascontiguousarray(user_value, dtype=np.int32)
    ptr = np.ascontiguousarray(value_ptr, dtype=np.int64)
    items = np.ascontiguousarray(value_items, dtype=np.int32)
    if uv.shape != (int(n_users),):
        raise ValueError('context values for %s users, %d expected' % (uv.shape, n_users))
    if ptr.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or ptr[-1] != len(items) or (np.diff(ptr) < 0).any():
        raise ValueError('value_ptr is not the row pointer of the %d list entries' % len(items))
    n_values = len(ptr) - 1
    if len(uv) and (uv.min() < -1 or uv.max() >= n_values):
        raise ValueError('user context values span [%d, %d]: outside -1..%d' % (uv.min(), uv.max(), n_values - 1))
    if len(items):
        if items.min() < 0 or items.max() >= n_items:
            raise ValueError('context items span [%d, %d]: outside the %d items' % (items.min(), items.max(), n_items))
        step_ok = np.diff(items.astype(np.int64)) > 0
        step_ok[ptr[1:-1][(ptr[1:-1] > 0) & (ptr[1:-1] < len(items))] - 1] = True      # a new value's list starts anywhere
        if not step_ok.all():
            raise ValueError('the items of a context value must be ascending and distinct')
    max_list = int(np.diff(ptr).max()) if n_values else 0
    return uv, ptr, (items if len(items) else np.zeros(1, dtype=np.int32)), max_list


class ItemPostFilteringMixin:
    """Mix in FRONT of a model served through `scoring.recommend` (the SVD family, the hybrids, the models with explicit user
    factors): `class ContextualSVD(ItemPostFilteringMixin, SVDModel)`, built on an `ItemPostFilteringArrayData`."""
    context_order_users = True      # workgroups of users with the same first-context value run next to each other

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._context_dev = None
        self._refuse_unsupported()

    def _refuse_unsupported(self):
        from .models import CoffeeModel, _DenseItemModel
        name = type(self).__name__
        if isinstance(self, _DenseItemModel):
            raise NotImplementedError('%s: contextual post-filtering is not built for the item-to-item / most-popular models '
                                      '(their lists do not come from the factor scoring pass)' % name)
        if isinstance(self, CoffeeModel):
            raise NotImplementedError('%s: contextual post-filtering is not built for tensor models' % name)
        if self.comm.world > 1:
            raise NotImplementedError('%s: contextual post-filtering is single-process (comm.world = %d)' % (name, self.comm.world))
        if not (hasattr(self.data, 'contexts') and hasattr(self.data, 'user_context') and hasattr(self.data, 'context_values')):
            raise TypeError('%s needs an ItemPostFilteringArrayData (the pandas ItemPostFilteringData is not accepted)' % name)

    # ---- the fused path ----------------------------------------------------------------------------------------------
    def get_recommendations(self):
        self._refuse_unsupported()
        self._tier_ran = False
        recs = super().get_recommendations()
        if len(recs) and not self._tier_ran:
            raise NotImplementedError('%s: its lists do not come from the factor scoring pass; contextual post-filtering '
                                      'does not compose with it' % type(self).__name__)
        return recs

    def _holdout_users(self):
        hold = self.data.test.holdout
        if hold is None:
            raise ValueError('contextual post-filtering needs a holdout (one row per test user)')
        return np.asarray(hold.userid)

    def _context_images(self, T, row_users):
        """(device images of the contexts in mapping order, int32 device order of the rows or None), cached: they belong to
        one serving order of the items, one mapped state of the data and one test matrix (whose rows `row_users()` names —
        asked only when the images are made: the protocol's host passes over the test entries cost more than the merge)"""
        data = self.data
        contexts = data.contexts
        users = [data.user_context(c) for c in contexts]            # (rebuilds the mapped state when an event dropped it)
        key = (self._item_rank, data.context_data, T)
        cached = self._context_dev
        if cached is not None and all(a is b for a, b in zip(cached[0], key)):
            return cached[1], cached[2]
        ops = self.ops
        n_items = int(data.n_items)
        hu = self._holdout_users()
        row_users = np.asarray(row_users(), dtype=np.int64)
        pos = np.minimum(np.searchsorted(hu, row_users), max(len(hu) - 1, 0))
        hit = (hu[pos] == row_users) if len(hu) else np.zeros(len(row_users), dtype=bool)
        images = []
        for c, uv in zip(contexts, users):
            _, ptr, items = data.context_values(c)
            if self._item_rank is not None:                          # serving positions, ascending within a value again
                value_of = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
                items = np.sort(value_of * n_items + self._item_rank[items]) % n_items
            rows_uv = np.where(hit, uv[pos], -1) if len(hu) else np.full(len(row_users), -1)
            images.append(ops.context_lists(rows_uv, ptr, items, len(row_users), n_items))
        order = None
        if self.context_order_users and images and len(row_users) > 1:
            first = np.where(hit, users[0][pos], -1) if len(hu) else np.full(len(row_users), -1)
            order = ops.to_device(np.argsort(first, kind='stable').astype(np.int32))
        self._context_dev = (key, images, order)
        return images, order

    def _list_tier(self, T, queries, row_users):
        ops = self.ops
        image = self._item_factors_device()
        contexts, order = self._context_images(T, row_users)
        self._tier_ran = True
        if not contexts:
            return queries, None
        # ONE block of query rows for both tiers: the pass scores with it (no fold-in of its own) and so does the merge
        E = queries if queries is not None else ops.spmm(T, image.fold_in)
        filter_seen = self.filter_seen

        def finish(recs_dev, stats):
            seen = (T.indptr, T.indices) if filter_seen else None
            out, cls = ops.context_merge(image.V, E, seen, contexts, recs_dev, want_class=bool(self.collect_recommend_stats),
                                         order=order)
            if cls is not None:
                stats['context_class'] = ops.to_host(cls)
            return out
        return E, finish

    # ---- the dense path (the reference's protocol) --------------------------------------------------------------------
    def upvote_context_items(self, context, scores, test_users):
        """contextual/models.py:5-24, IN PLACE on the host block `scores` [len(test_users) x n_items] (the data's item ids):
        every (user, item of the user's value of `context`) becomes max(scores) + score + 1."""
        if context is None:
            return
        _, ptr, items = self.data.context_values(context)
        uv = self.data.user_context(context)
        hu = self._holdout_users()
        test_users = np.asarray(test_users, dtype=np.int64)
        pos = np.minimum(np.searchsorted(hu, test_users), max(len(hu) - 1, 0))
        val = np.where(hu[pos] == test_users, uv[pos], -1) if len(hu) else np.full(len(test_users), -1)
        has = np.flatnonzero(val >= 0)
        counts = ptr[val[has] + 1] - ptr[val[has]]
        if not counts.sum():
            return
        rows = np.repeat(has, counts)
        start = np.repeat(ptr[val[has]], counts)
        cols = items[start + (np.arange(len(rows)) - np.repeat(np.cumsum(counts) - counts, counts))]
        scores[rows, cols] = scores.max() + scores[rows, cols] + 1

    def upvote_relevant_items(self, scores, test_users):
        """contextual/models.py:26-28: context by context in mapping order, each with the maximum of the block as the
        earlier ones left it"""
        for context in self.data.contexts:
            self.upvote_context_items(context, scores, test_users)

    def slice_recommendations(self, test_data, shape, start, stop, test_users=None):
        self._refuse_unsupported()
        scores, slice_data = super().slice_recommendations(test_data, shape, start, stop, test_users)
        if test_users is None:
            test_users = self._get_test_data()[2]
        self.upvote_relevant_items(scores, np.asarray(test_users)[start:min(stop, shape[0])])
        return scores, slice_data
