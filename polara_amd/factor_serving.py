"""Serving for models that carry explicit user factors (ProbabilisticMF, ImplicitALS, ImplicitBPR, LCEModel, LightFMWrapper):
the rows of the user factors go into the scoring pass as ready-made queries (`scoring.recommend(queries=...)`), and
`slice_recommendations` is the dense product of those rows with the item factors.  A build ends with `_set_factors`, which
leaves `factors` ({userid: host array, itemid: host array, ...}), `_factors_dev` ((host user factors, their device copy, then
what `_extra_factors_device` names) or None), `_item_inv` and the item image of `_item_factors_device`; the model provides
`_rank`."""
import numpy as np

from . import scoring


class FactorQueriesMixin:
    @property
    def rank(self):
        return self._rank

    @rank.setter
    def rank(self, new_value):
        # the factors of these models are not nested: no truncation, a rank change invalidates the model
        if new_value != self._rank:
            self._rank = new_value
            self._is_ready = False
            self._recommendations = None
            self._factor_image = None

    def _training_device_csr(self):
        """what these models factorise: the training matrix in the data's own item order"""
        return self._data_order_training_csr()

    def _clean_metadata(self):
        """the data changed (every model subscribes this in its `__init__`): what the last build left on the device is stale"""
        self._factors_dev = None

    def _set_factors(self, P, Q, kept=(), **named):
        """The tail of a build from the device blocks P (users) and Q (items, the data's item order): `factors` on the host —
        with f'{itemid}_{name}' for every further device block `named` —, `_factors_dev` with the blocks `kept` on the device
        behind P (what `_extra_factors_device` uploads again), and the serving index over Q."""
        userid, itemid = self.data.fields.userid, self.data.fields.itemid
        to_host = self.ops.to_host
        self.factors = {userid: to_host(P), itemid: to_host(Q), **{f'{itemid}_{name}': to_host(X) for name, X in named.items()}}
        self._factors_dev = (self.factors[userid], P, *kept)
        self._set_item_serving_index(Q)

    def _extra_factors_device(self):
        """uploads of further `factors` that stay on the device with the user factors (the tail of `_factors_dev`)"""
        return ()

    def _user_factors_block(self):
        """P [n_users x k] on the device: the block of the build, or an upload when `factors` was swapped"""
        P = self.factors.get(self.data.fields.userid, None)
        if P is None:
            raise ValueError('%s: no user factors (build the model first)' % self.method)
        kept = self._factors_dev
        if kept is None or kept[0] is not P:
            kept = self._factors_dev = (P, self.ops.to_device(np.ascontiguousarray(P, dtype=np.float64)),
                                        *self._extra_factors_device())
        return kept[1]

    def _user_rows(self, users):
        """rows `users` of P with an even leading dimension (what the sweep reads its queries' rows at)"""
        ops = self.ops
        P = self._user_factors_block()
        k = int(P.shape[1])
        block = ops.zeros(len(users), k + (k & 1))
        block[:, :k] = P[ops.to_device(np.ascontiguousarray(users, dtype=np.int64))]
        return block[:, :k]

    def _check_serving(self):
        """what the model refuses to serve, before any work"""
        if self.data.warm_start:
            raise NotImplementedError('%s has no warm start' % self.method)

    def _test_queries(self, test_users, start=0, stop=None):
        """the query rows of test users [start, stop) — a device fp64 block with an even leading dimension"""
        return self._user_rows(np.asarray(test_users)[start:stop])

    def get_recommendations(self):
        self._check_serving()
        if self.verify_integrity:
            self.verify_data_integrity()
        ops = self.ops
        T, n_users, n_items = self._device_test_csr()
        test_users = np.asarray(self._get_test_data()[2], dtype=np.int64)
        if len(test_users) != n_users:
            raise ValueError('%d test users, the test matrix has %d rows' % (len(test_users), n_users))
        if n_users == 0:
            return np.empty((0, self.topk), dtype=np.int64)
        stats = {}
        queries, finish = self._list_tier(T, self._test_queries(test_users), lambda: test_users)
        recs_dev = scoring.recommend(ops, self._item_factors_device(), T, self.topk, self.filter_seen,
                                     stats=stats if self.collect_recommend_stats else None, queries=queries)
        if finish is not None:
            recs_dev = finish(recs_dev, stats)
        self.recommend_stats = stats
        recs = self._external_ids(recs_dev, self._item_inv)
        self._recs_dev = (recs, recs_dev)
        return recs

    def slice_recommendations(self, test_data, shape, start, stop, test_users=None):
        """The dense fp64 scores of test users [start, stop) against every item (external item order) and the slice triplet."""
        if test_users is None:
            test_users = self._get_test_data()[2]
        stop = min(stop, shape[0])
        slice_data = self._slice_test_data(test_data, start, stop)
        image = self._item_factors_device()
        E = self._test_queries(test_users, start, stop).contiguous()
        scores = self.ops.to_host(self.ops.dense_scores(image.V, E))
        out = np.empty_like(scores)
        out[:, self._item_inv] = scores
        return out, slice_data
