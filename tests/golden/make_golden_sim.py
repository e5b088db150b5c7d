"""Generates tests/golden/sim_*.npz and tests/golden/simcs_*.npz from the REFERENCE ITSELF: the unmodified
`SimilarityAggregation` (hybrid/models.py:25-44) and `SimilarityAggregationItemColdStart` (coldstart/models.py:101-119) of
evfro/polara driven on seeded data through `SimilarityDataModel` / `ItemColdStartSimilarityData`, with the item similarity
from the reference's own `polara.lib.similarity` (cosine similarity of seeded one-hot features: non-dyadic values).

Runs only in the build container (imports the reference from /root/reference through the test-only numba, scikit-sparse and
lightfm stand-ins, like make_golden_coldstart.py).  One in-memory adjustment, for the generation only, the one of
make_golden_i2i.py: the sparse case of the reference's `downvote_seen_items` ends in `recs -= seen_recs`, which rebinds a
local name, so filter_seen has no effect in the sparse branch; here that line runs in place, and every fixture records whether
that changed its lists (`sparse_downvote_changed`) next to the lists of the unmodified code (`recs_unmodified`).

Stored: the inputs as the hot path sees them (training and test triplets, S as triplets after the data object's diagonal
treatment, for SIM(cs) the cold similarity as triplets in the reference's stored order plus the holdout), the settings, the reference's lists and the dense
scores of a few rows.

Conditions asserted before anything is written: a sparse-branch fixture either keeps the reference's product sparse or
has at least `topk` candidates with a positive score in every row and no negative score (so the reference's silent
conversion to dense cannot change a list); every SIM fixture has at least 50 test rows; the fixtures hold the cases they
are named after (pads, zero-feedback entries, different lists in the two branches of a non-symmetric S).

usage:  python tests/golden/make_golden_sim.py
"""
import contextlib
import io
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for shim in ('_lightfm_shim', '_sksparse_shim', '_numba_shim'):
    sys.path.insert(0, os.path.join(HERE, shim))
sys.path.insert(0, '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
warnings.filterwarnings('ignore')

import numpy as np
import pandas as pd
import scipy.sparse as sps

from polara.recommender.models import RecommenderModel
from polara.recommender.hybrid.data import SimilarityDataModel
from polara.recommender.hybrid.models import SimilarityAggregation
from polara.recommender.coldstart.data import ItemColdStartSimilarityData
from polara.recommender.coldstart.models import SimilarityAggregationItemColdStart
from polara.lib.similarity import stack_features, cosine_similarity
from polara.lib.sparse import sparse_dot

import i2i_reference as ref
import sim_reference as sim

SCORE_ROWS = 6
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


def ratings(n_users, n_items, lo, hi, seed, zeros=False):
    """Users with lo..hi-1 distinct uniformly drawn items, ratings 1..5 (with `zeros`: a fifth of them 0, a seventh negative)."""
    rng = np.random.RandomState(seed)
    rows = []
    for u in range(n_users):
        for it in rng.choice(n_items, rng.randint(lo, hi), replace=False):
            v = float(rng.randint(1, 6))
            if zeros:
                x = rng.rand()
                v = 0.0 if x < 0.2 else (-v if x < 0.35 else v)
            rows.append((u, int(it), v))
    return pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])


def features(n_items, n_labels, seed, most=5):
    """one list of 1..most seeded labels per item"""
    rng = np.random.RandomState(seed)
    rows = [sorted(int(x) for x in rng.choice(n_labels, rng.randint(1, most + 1), replace=False)) for _ in range(n_items)]
    return pd.DataFrame({'genres': rows}, index=pd.Index(np.arange(n_items), name='itemid'))


def similarity(feat, row_scaling_seed=None):
    F, _ = stack_features(feat, normalize=False)
    S = cosine_similarity(F.tocsr().astype(np.float64)).tocsr()
    if row_scaling_seed is not None:            # a non-symmetric S: row i scaled by one of 0.5, 0.6, ..., 1.4
        d = np.random.RandomState(row_scaling_seed).randint(5, 15, S.shape[0]) / 10.0
        S = sps.diags(d).dot(S).tocsr()
    return S


def candidates_survive_a_dense_conversion(scores, seen, topk):
    """every row has at least topk unseen positive scores and no negative one: the dense selection then returns the
    sparse branch's list"""
    s = np.asarray(scores.toarray() if sps.issparse(scores) else scores)
    return bool((s >= 0).all() and (((s > 0) & ~seen).sum(axis=1) >= topk).all())


def run_sim(data, topk, filter_seen, dense_output, implicit):
    model = SimilarityAggregation(data)
    model.verbose = False
    model.topk, model.filter_seen, model.dense_output, model.implicit = topk, filter_seen, dense_output, implicit
    quiet(model.build)
    test_data, test_shape, _ = model._get_test_data()
    scores, _ = model.slice_recommendations(test_data, test_shape, 0, test_shape[0])
    RecommenderModel.downvote_seen_items = staticmethod(_ref_downvote)
    unmodified = np.asarray(model.get_recommendations(), np.int64)
    RecommenderModel.downvote_seen_items = staticmethod(_downvote_in_place)
    model._recommendations = None
    recs = np.asarray(model.get_recommendations(), np.int64)
    RecommenderModel.downvote_seen_items = staticmethod(_ref_downvote)
    return model, test_data, test_shape, scores, recs, unmodified


def sim_fixture(name, df, S, topk=10, warm_start=False, filter_seen=True, dense_output=False, implicit=False,
                expect_sparse=None, both_branches=False, expect_pads=None, expect_changed=None):
    n_items = S.shape[0]
    data = SimilarityDataModel(df, 'userid', 'itemid', 'rating', seed=0, relations_matrices={'itemid': S, 'userid': None},
                               relations_indices={'itemid': np.arange(n_items), 'userid': None})
    data.verbose = False
    data.warm_start = warm_start
    data.holdout_size = 1
    data.test_ratio, data.test_fold = 0.5, 2          # half of the users are test users: 60-100 rows survive the filters
    quiet(data.prepare)
    model, test_data, test_shape, scores, recs, unmodified = run_sim(data, topk, filter_seen, dense_output, implicit)
    assert test_shape[0] >= 50, (name, test_shape)
    tu, ti, tf = test_data
    seen = np.zeros(tuple(test_shape[:2]), dtype=bool)
    seen[tu, ti] = filter_seen
    if not dense_output:
        if expect_sparse is not None:
            assert sps.issparse(scores) == expect_sparse, (name, type(scores))
        assert sps.issparse(scores) or candidates_survive_a_dense_conversion(scores, seen, topk), name
    idx, val, shp = data.to_coo(tensor_mode=False, feedback_threshold=model.feedback_threshold)
    rel = data.get_relations_matrix('itemid').tocoo()
    dense_rows = np.asarray(scores[:SCORE_ROWS].toarray() if sps.issparse(scores) else scores[:SCORE_ROWS], np.float64)
    out = dict(model=np.str_(model.method), train_idx=idx.astype(np.int64), train_val=np.asarray(val, np.float64),
               train_shape=np.array(shp, np.int64), test_user=np.asarray(tu, np.int64), test_item=np.asarray(ti, np.int64),
               test_fdbk=np.asarray(tf, np.float64), test_shape=np.array(test_shape, np.int64), topk=np.int64(topk),
               filter_seen=np.bool_(filter_seen), dense_output=np.bool_(dense_output), implicit=np.bool_(implicit),
               warm_start=np.bool_(warm_start), s_row=rel.row.astype(np.int32), s_col=rel.col.astype(np.int32),
               s_val=rel.data.astype(np.float64), recs=recs, recs_unmodified=unmodified,
               sparse_downvote_changed=np.bool_(not np.array_equal(recs, unmodified)),
               score_rows=np.arange(len(dense_rows), dtype=np.int64), scores=dense_rows)
    if both_branches:
        _, _, _, o_scores, o_recs, _ = run_sim(data, topk, filter_seen, not dense_output, implicit)
        out['recs_other'] = o_recs
        assert not np.array_equal(o_recs, recs), name + ': the two branches of a non-symmetric S give the same lists'
    # the fixture holds the case it is named after, and the restatement reads it as the reference did
    pads = int((recs < 0).sum())
    if expect_pads is not None:
        assert (pads > 0) == expect_pads, (name, pads)
    if expect_changed is not None:
        assert bool(out['sparse_downvote_changed']) == expect_changed, name
    if implicit:
        assert (out['test_fdbk'] == 0).any() and (out['test_fdbk'] < 0).any(), name + ': no zero or no negative test feedback'
    r_scores, r_cls, r_lists = sim.sim_lists(out)
    assert np.array_equal(r_scores[:len(dense_rows)], dense_rows), name + ': restated scores differ from the reference\'s'
    assert ref.tie_aware_mismatches(r_lists, recs, r_scores, r_cls) == [], name
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-16s test %s, S fill %.2f %%, product fill %.1f %% (%s), pads %d, changed by the in-place downvote: %s, %d bytes'
          % (name, tuple(test_shape), 100.0 * rel.nnz / float(shp[1]) ** 2, 100.0 * np.count_nonzero(r_scores) / r_scores.size,
             'sparse' if sps.issparse(scores) else 'dense', pads, out['sparse_downvote_changed'], os.path.getsize(path)))


def simcs_fixture(name, df, feat, topk=10, implicit=False, expect_sparse=None, expect_pads=None, data_seed=7):
    S = similarity(feat)
    data = ItemColdStartSimilarityData(df, 'userid', 'itemid', 'rating', seed=data_seed, item_features=feat,
                                       relations_matrices={'itemid': S, 'userid': None},
                                       relations_indices={'itemid': feat.index.values, 'userid': None})
    data.verbose = False
    quiet(data.prepare)
    # the holdout's keys as row numbers of the lists (see make_golden_coldstart.py)
    new = data.index.itemid.cold_start.new.values
    if not np.array_equal(new, np.arange(len(new))):
        pos = pd.Series(np.arange(len(new)), index=new)
        hold = data.test.holdout
        hold['itemid_cold'] = hold['itemid_cold'].map(pos).values
    model = SimilarityAggregationItemColdStart(data)
    model.verbose = False
    model.topk, model.implicit = topk, implicit
    quiet(model.build)
    recs = np.asarray(model.get_recommendations(), np.int64)
    cold = sps.csr_matrix(data.cold_items_similarity)
    A = model.get_training_matrix()
    if implicit:
        A.data = np.ones_like(A.data)
    scores = sparse_dot(cold, A, False, True)
    if expect_sparse is not None:
        assert sps.issparse(scores) == expect_sparse, (name, type(scores))
    nothing_seen = np.zeros(scores.shape, dtype=bool)
    assert sps.issparse(scores) or candidates_survive_a_dense_conversion(scores, nothing_seen, topk), name
    dense_rows = np.asarray(scores[:SCORE_ROWS].toarray() if sps.issparse(scores) else scores[:SCORE_ROWS], np.float64)
    idx, val, shp = data.to_coo(tensor_mode=False)
    hold = data.test.holdout
    c = cold.tocoo()
    out = dict(model=np.str_(model.method), train_idx=idx.astype(np.int64), train_val=np.asarray(val, np.float64),
               train_shape=np.array(shp, np.int64), cold_row=c.row.astype(np.int32), cold_col=c.col.astype(np.int32),
               cold_val=c.data.astype(np.float64), cold_shape=np.array(cold.shape, np.int64),
               hold_user=hold['userid'].values.astype(np.int64), hold_cold=hold['itemid_cold'].values.astype(np.int64),
               hold_fdbk=hold['rating'].values.astype(np.float64), topk=np.int64(topk), implicit=np.bool_(implicit),
               dense_output=np.bool_(False), filter_seen=np.bool_(False), recs=recs,
               score_rows=np.arange(len(dense_rows), dtype=np.int64), scores=dense_rows)
    pads = int((recs < 0).sum())
    if expect_pads is not None:
        assert (pads > 0) == expect_pads, (name, pads)
    r_scores, r_cls, r_lists = sim.simcs_lists(out)
    # (the reference's cold similarity comes out of two fancy-indexing steps and its rows are NOT sorted by column; the
    # triplets are stored in that order, because SciPy's product adds in the stored order and other orders differ in the
    # last bits)
    assert np.array_equal(r_scores[:len(dense_rows)], dense_rows), name + ': restated scores differ from the reference\'s'
    assert ref.tie_aware_mismatches(r_lists, recs, r_scores, r_cls) == [], name
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-16s cold %s, product fill %.1f %% (%s), pads %d in %d rows, %d bytes'
          % (name, tuple(cold.shape), 100.0 * np.count_nonzero(r_scores) / r_scores.size,
             'sparse' if sps.issparse(scores) else 'dense', pads, int((recs < 0).any(axis=1).sum()), os.path.getsize(path)))


def first_seed(make, seeds, what):
    """seeds are tried in order until the fixture meets its conditions"""
    for s in seeds:
        try:
            return make(s)
        except AssertionError as exc:
            print('%s: seed %d rejected: %s' % (what, s, exc))
    raise SystemExit('%s: no seed met the conditions' % what)


def main():
    big = ratings(400, 3000, 3, 9, seed=1)
    S_big = similarity(features(3000, 300, seed=2, most=3))
    sim_fixture('sim_sparse', big, S_big, topk=50, expect_sparse=True, expect_pads=True, expect_changed=True)
    sim_fixture('sim_nofilter', big, S_big, filter_seen=False, expect_sparse=True)
    sim_fixture('sim_warm', big, S_big, warm_start=True, expect_sparse=True)
    sim_fixture('sim_implicit', ratings(400, 3000, 3, 9, seed=3, zeros=True), S_big, implicit=True, expect_sparse=True)
    small = ratings(300, 200, 4, 15, seed=4)
    sim_fixture('sim_dense', small, similarity(features(200, 40, seed=5)), dense_output=True, topk=20)
    sim_fixture('sim_nonsym', big, similarity(features(3000, 300, seed=2, most=3), row_scaling_seed=6), expect_sparse=True,
                both_branches=True)
    cs_df, cs_feat = ratings(400, 600, 6, 30, seed=11), features(600, 300, seed=12)
    simcs_fixture('simcs_sparse', cs_df, cs_feat, expect_sparse=True, expect_pads=True)
    simcs_fixture('simcs_implicit', cs_df, cs_feat, implicit=True, expect_sparse=True)
    first_seed(lambda s: simcs_fixture('simcs_full', ratings(300, 150, 6, 30, seed=s), features(150, 40, seed=s + 1),
                                       expect_pads=False), range(21, 60), 'simcs_full')


if __name__ == '__main__':
    main()
