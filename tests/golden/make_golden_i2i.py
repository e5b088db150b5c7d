"""Generates tests/golden/i2i_*.npz and tests/golden/mp_*.npz from the REFERENCE ITSELF: the unmodified
`CooccurrenceModel` and `PopularityModel` of evfro/polara (models.py:649-725) driven on small seeded data through
`RecommenderData`, their item-to-item matrix and their lists stored next to the inputs the hot path sees.

Runs only in the build container (imports the reference from /root/reference through the test-only numba shim, like
make_golden.py).  One in-memory adjustment, for the generation only: the sparse case of the reference's
`downvote_seen_items` (models.py:494-510) ends in `recs -= seen_recs`, which rebinds the function's local name — SciPy
matrices have no in-place subtraction — so the caller's score matrix keeps its seen entries and filter_seen has no
effect in the sparse branch.  Here that one line runs in place (the matrix the caller holds loses its seen entries, as
the reference's comment says it should); every fixture records whether that changed its lists
(`sparse_downvote_changed`), next to the lists of the unmodified code (`recs_unmodified`).

usage:  python tests/golden/make_golden_i2i.py
"""
import contextlib
import io
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, '_numba_shim'))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')

import numpy as np
import pandas as pd
import scipy.sparse as sps

from polara import RecommenderData
from polara.recommender.models import CooccurrenceModel, PopularityModel, RecommenderModel

_ref_downvote = RecommenderModel.downvote_seen_items


def _downvote_in_place(recs, idx_seen):
    if sps.issparse(recs):
        idx_seen = idx_seen[:2]
        seen = sps.coo_matrix((np.ones(len(idx_seen[0]), dtype=bool), idx_seen), shape=recs.shape)
        new = (recs - recs.multiply(seen)).tocsr()
        recs.data, recs.indices, recs.indptr = new.data, new.indices, new.indptr
    else:
        _ref_downvote(recs, idx_seen)


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def sparse_frame(n_users, n_items, lo, hi, seed, step=1.0, levels=5, negative=False):
    """Users with lo..hi-1 distinct uniformly drawn items: a co-occurrence product that stays sparse."""
    rng = np.random.RandomState(seed)
    rows = []
    for u in range(n_users):
        items = rng.choice(n_items, rng.randint(lo, hi), replace=False)
        for it in items:
            v = rng.randint(1, levels + 1) * step
            if negative and rng.rand() < 0.2:
                v = -v
            rows.append((u, int(it), v))
    return pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])


def fixture(name, df, model_cls, topk=10, warm_start=False, filter_seen=True, dense_output=False, implicit=False,
            by_feedback_value=False, expect_sparse=None, holdout_size=3):
    data = RecommenderData(df, 'userid', 'itemid', 'rating', seed=0)
    data.verbose = False
    data.warm_start = warm_start
    data.holdout_size = holdout_size
    quiet(data.prepare)
    model = model_cls(data)
    model.verbose = False
    model.topk = topk
    model.filter_seen = filter_seen
    if model_cls is CooccurrenceModel:
        model.dense_output = dense_output
        model.implicit = implicit
    else:
        model.by_feedback_value = by_feedback_value
    quiet(model.build)
    test_data, test_shape, _ = model._get_test_data()
    if expect_sparse is not None:
        scores, _ = model.slice_recommendations(test_data, test_shape, 0, test_shape[0])
        assert sps.issparse(scores) == expect_sparse, (name, type(scores))
    RecommenderModel.downvote_seen_items = staticmethod(_ref_downvote)
    unmodified = model.get_recommendations()
    RecommenderModel.downvote_seen_items = staticmethod(_downvote_in_place)
    model._recommendations = None
    recs = model.get_recommendations()
    RecommenderModel.downvote_seen_items = staticmethod(_ref_downvote)

    idx, val, shp = data.to_coo(tensor_mode=False, feedback_threshold=model.feedback_threshold)
    tu, ti, tf = test_data
    out = dict(model=np.str_(model.method), train_idx=idx.astype(np.int64), train_val=np.asarray(val, np.float64),
               train_shape=np.array(shp, np.int64), test_user=np.asarray(tu, np.int64), test_item=np.asarray(ti, np.int64),
               test_fdbk=np.asarray(tf, np.float64), test_shape=np.array(test_shape, np.int64), topk=np.int64(topk),
               filter_seen=np.bool_(filter_seen), dense_output=np.bool_(dense_output), implicit=np.bool_(implicit),
               by_feedback_value=np.bool_(by_feedback_value), warm_start=np.bool_(warm_start),
               recs=np.asarray(recs, np.int64), recs_unmodified=np.asarray(unmodified, np.int64),
               sparse_downvote_changed=np.bool_(not np.array_equal(recs, unmodified)))
    if model_cls is CooccurrenceModel:
        C = model._i2i_matrix.tocoo()
        out.update(c_row=C.row.astype(np.int32), c_col=C.col.astype(np.int32), c_val=C.data.astype(np.float64))
    else:
        out.update(item_scores=np.asarray(model.item_scores, np.float64))
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-16s test %s, pads %d, changed by the in-place downvote: %s, %d bytes'
          % (name, tuple(test_shape), int((recs < 0).sum()), out['sparse_downvote_changed'], os.path.getsize(path)))


def main():
    sparse = sparse_frame(400, 3000, 3, 9, seed=1)
    fixture('i2i_sparse', sparse, CooccurrenceModel, expect_sparse=True)
    fixture('i2i_nofilter', sparse, CooccurrenceModel, filter_seen=False, expect_sparse=True)
    fixture('i2i_warm', sparse, CooccurrenceModel, warm_start=True, expect_sparse=True)
    fixture('i2i_implicit', sparse_frame(400, 3000, 3, 9, seed=2, negative=True), CooccurrenceModel, implicit=True,
            expect_sparse=True)
    small = sparse_frame(300, 200, 4, 15, seed=3, negative=True)
    fixture('i2i_dense', small, CooccurrenceModel, dense_output=True, topk=20)
    fixture('i2i_nondyadic', sparse_frame(300, 200, 4, 15, seed=4, step=0.1, levels=10), CooccurrenceModel,
            dense_output=True, topk=20)
    pop = sparse_frame(300, 120, 4, 30, seed=5)
    fixture('mp_count', pop, PopularityModel, topk=15)
    fixture('mp_feedback', pop, PopularityModel, topk=15, by_feedback_value=True)


if __name__ == '__main__':
    main()
