"""Generates tests/golden/sampled_*.npz from the REFERENCE ITSELF: the unmodified `SVDModel` of evfro/polara under its own
`RandomSampleEvaluationSVDMixin` (models.py:1095-1183), fed by `RecommenderData` under `RandomSampleEvaluationMixin`
(data.py:938-994), on seeded data with explicit `unseen_interactions`.

Runs only in the build container (imports the reference from /root/reference through the test-only numba stand-in, like
make_golden_sim.py; `inner_product_at` then runs as the Python loop it is written as).  One in-memory adjustment for the
generation only, the one of make_golden.py: the reference's `safe_divide` gets a zero-initialised output, without which
precision / recall / nDCG come out of uninitialised memory.

Stored: the training and test triplets as the hot path sees them, the holdout (users as row numbers of the lists), the unseen
lists, the reference's V, the folded-in user factors, the full `[holdout | unseen]` score matrix, the reference's lists, its
`evaluate('relevance')`, `('ranking')` and `('hits')` outputs and, per row, `min_gap`: the smallest difference between
consecutive values of the sorted top-(k+1) scores.

Asserted before anything is written: every row has min_gap > 1e-6 * max|score| (else the next seed is tried), so every row
takes part in list comparisons; the restatement of tests/sampled_reference.py gives the reference's scores bit for bit and
its lists.

The sampled path (`compute_random_item_scores_gen`) is not covered: its stream is numba's, which is not on this machine.

usage:  python tests/golden/make_golden_sampled.py
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

from polara.recommender.data import RecommenderData, RandomSampleEvaluationMixin
from polara.recommender.models import SVDModel, RandomSampleEvaluationSVDMixin
import polara.recommender.evaluation as _ref_evaluation

import sampled_reference as ref


def _safe_divide_zero_init(a, b, mask=None, dtype=None):
    pos = mask if mask is not None else a > 0
    out = np.zeros(np.broadcast(np.asarray(a), np.asarray(b)).shape, dtype=dtype or np.float64)
    return np.divide(a, b, out=out, where=pos)


_ref_evaluation.safe_divide = _safe_divide_zero_init


class SampledData(RandomSampleEvaluationMixin, RecommenderData):
    pass


class SampledSVD(RandomSampleEvaluationSVDMixin, SVDModel):
    pass


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def ratings(n_users, n_items, lo, hi, seed):
    rng = np.random.RandomState(seed)
    rows = []
    for u in range(n_users):
        for it in rng.choice(n_items, rng.randint(lo, hi), replace=False):
            rows.append((u, int(it), float(rng.randint(1, 6))))
    return pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])


def metric_arrays(model, out):
    for kind in ('relevance', 'ranking', 'hits'):
        score = model.evaluate(kind)
        out['metric_%s_names' % kind] = np.array(score._fields)
        out['metric_%s' % kind] = np.array([np.float64(x) for x in score], dtype=np.float64)    # (None -> NaN)


def fixture(name, seed, holdout_size, warm_start, n_unseen, rank=10, topk=10):
    df = ratings(200, 400, 12, 40, seed)
    data = SampledData(df, 'userid', 'itemid', 'rating', seed=seed)
    data.verbose = False
    data.warm_start = warm_start
    data.holdout_size = holdout_size
    data.test_ratio, data.test_fold = 0.5, 2
    quiet(data.prepare)
    userid, itemid = data.fields.userid, data.fields.itemid
    model = SampledSVD(data)
    model.verbose = False
    model.rank, model.topk = rank, topk
    (tu, ti, tf), tshape, _ = model._get_test_data()
    hold = data.test.holdout
    hold_users = hold[userid].values
    test_users = hold[userid].drop_duplicates().values
    assert len(test_users) == tshape[0] and 80 <= tshape[0] <= 120, (name, tshape, len(test_users))
    hold_row = pd.factorize(hold_users, sort=False)[0].astype(np.int64)
    hold_item = hold[itemid].values.astype(np.int64)
    # unseen lists: seeded draws from the items outside the user's test row and holdout
    rng = np.random.RandomState(seed + 1000)
    unseen = np.empty((tshape[0], n_unseen), dtype=np.int64)
    for r in range(tshape[0]):
        taken = np.union1d(ti[tu == r], hold_item[hold_row == r])
        unseen[r] = rng.choice(np.setdiff1d(np.arange(tshape[1]), taken), n_unseen, replace=False)
    data.set_unseen_interactions(pd.Series(list(unseen), index=pd.Index(test_users, name=userid)), reindex=False)
    np.random.seed(seed)
    quiet(model.build)
    recs = np.asarray(model.get_recommendations(), dtype=np.int64)
    V = model.factors[itemid]
    test_matrix, _ = model.get_test_matrix()
    user_factors = test_matrix.dot(V)
    scores = np.concatenate((model.compute_holdout_scores(user_factors, V),
                             model.compute_random_item_scores(user_factors, V)), axis=1)
    top = -np.sort(-scores, axis=1)[:, :topk + 1]
    min_gap = (top[:, :-1] - top[:, 1:]).min(axis=1)
    assert (min_gap > 1e-6 * np.abs(scores).max()).all(), '%s: a near-tie in the top-%d of a row' % (name, topk + 1)
    idx, val, shp = data.to_coo(tensor_mode=False)
    out = dict(train_idx=idx.astype(np.int64), train_val=np.asarray(val, np.float64), train_shape=np.array(shp, np.int64),
               test_user=np.asarray(tu, np.int64), test_item=np.asarray(ti, np.int64), test_fdbk=np.asarray(tf, np.float64),
               test_shape=np.array(tshape, np.int64), hold_user=hold_row, hold_item=hold_item,
               hold_fdbk=hold[data.fields.feedback].values.astype(np.float64), unseen=unseen,
               V=np.ascontiguousarray(V, dtype=np.float64), user_factors=np.ascontiguousarray(user_factors, dtype=np.float64),
               scores=scores.astype(np.float64), recs=recs, min_gap=min_gap, topk=np.int64(topk), rank=np.int64(rank),
               holdout_size=np.int64(holdout_size), warm_start=np.bool_(warm_start), seed=np.int64(seed))
    metric_arrays(model, out)
    # the restatement reads the fixture as the reference did
    cand = np.concatenate((hold_item.reshape(-1, holdout_size), unseen), axis=1)
    r_lists, r_scores = ref.candidates_topk(user_factors, V, cand, topk)
    assert np.array_equal(r_scores, scores), name + ': restated scores differ from the reference\'s'
    assert np.array_equal(r_lists, recs), name + ': restated lists differ from the reference\'s'
    known = bool(np.isin(test_users, np.unique(idx[:, 0])).all()) if not warm_start else False
    assert warm_start or known, name + ': test users outside the training users'
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-14s test %s, %d + %d candidates, min gap %.2e (max |score| %.2e), %s, %d bytes'
          % (name, tuple(tshape), holdout_size, n_unseen, min_gap.min(), np.abs(scores).max(),
             ', '.join('%s %s' % (k[7:], np.round(out[k], 4).tolist()) for k in ('metric_relevance', 'metric_ranking')),
             os.path.getsize(path)))


def first_seed(make, seeds, what):
    for s in seeds:
        try:
            return make(s)
        except AssertionError as exc:
            print('%s: seed %d rejected: %s' % (what, s, exc))
    raise SystemExit('%s: no seed met the conditions' % what)


def main():
    first_seed(lambda s: fixture('sampled_h1', s, 1, True, 29), range(1, 40), 'sampled_h1')
    first_seed(lambda s: fixture('sampled_h3', s, 3, True, 27), range(41, 80), 'sampled_h3')
    first_seed(lambda s: fixture('sampled_known', s, 1, False, 29), range(81, 120), 'sampled_known')


if __name__ == '__main__':
    main()
