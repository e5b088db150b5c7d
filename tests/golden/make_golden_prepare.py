"""Generates tests/golden/prepare_*.npz from the REFERENCE ITSELF: the unmodified `RecommenderData.prepare()` of
evfro/polara (data.py:232-252) on seeded raw interactions — external ids with gaps, rows shuffled, five feedback levels
with many ties, users of very different lengths.

Runs only in the build container (imports the reference from /root/reference through the test-only numba stand-in, like
make_golden_sampled.py).  Nothing of the reference is changed.

Stored per case: the input columns, the configuration (JSON), the training triplets in their order, both user indices and
the item index (external ids in the order of their new numbers), the testset and the holdout as the reference left them
(sorted by user; the order inside a user is the reference's unstable sort's), holdout_size.

Asserted before anything is written: the new numbers of every index are 0, 1, 2, ...; the restatement of
tests/prepare_reference.py gives the training rows, all three indices and, per user, the rows of testset and holdout —
which includes rule 7 of DESIGN.md §8r (the order of the test users); on `prepare_order`, that sampling the testset AFTER
the filters would have given other rows than the reference's sampling before them.

usage:  python tests/golden/make_golden_prepare.py [--time]
"""
import contextlib
import io
import json
import os
import sys
import time
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

from polara.recommender.data import RecommenderData

import prepare_reference as twin


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def raw(n_users=400, n_items=150, seed=7, with_order=False):
    """a planted matrix: users of 2 .. 60 rows, ratings 1 .. 5 that follow a user x item pattern (many ties), external ids
    with gaps, rows shuffled"""
    rng = np.random.RandomState(seed)
    user_ids = np.sort(rng.choice(10 * n_users, n_users, replace=False)) + 1000
    item_ids = np.sort(rng.choice(10 * n_items, n_items, replace=False)) + 50
    rows = []
    for u in range(n_users):
        length = int(rng.choice([2, 3, 4, 6, 9, 15, 25, 40, 60], p=[.08, .08, .08, .16, .2, .2, .1, .06, .04]))
        for it in rng.choice(n_items, length, replace=False):
            rating = 1 + (u % 5 + it % 3 + rng.randint(0, 3)) % 5
            rows.append((user_ids[u], item_ids[it], float(rating)))
    df = pd.DataFrame(rows, columns=['userid', 'itemid', 'rating'])
    df = df.sample(frac=1, random_state=rng).reset_index(drop=True)
    if with_order:
        df['when'] = rng.permutation(len(df)).astype(np.int64) // 3 + 10 ** 9          # a timestamp with ties
    return df


def reference_split(df, config, custom_order=None):
    data = RecommenderData(df, 'userid', 'itemid', 'rating', custom_order=custom_order, seed=0)
    data.verbose = False
    data.verify_sessions_length_distribution = False
    for name, value in config.items():
        setattr(data, name, value)
    quiet(data.prepare)
    cols = ['userid', 'itemid', 'rating']

    def trip(frame):
        if frame is None:
            return None
        return tuple(frame[c].values.astype(np.float64 if c == 'rating' else np.int64) for c in cols)

    def index(frame):
        if frame is None:
            return None
        assert np.array_equal(frame['new'].values, np.arange(len(frame)))
        return frame['old'].values.astype(np.int64)
    return dict(training=trip(data.training), train_users=index(data.index.userid.training),
                test_users=index(data.index.userid.test), items=index(data.index.itemid),
                testset=trip(data.test.testset), holdout=trip(data.test.holdout), holdout_size=data.holdout_size), data


def user_sets(trip):
    """{user: sorted (item, feedback) rows}"""
    out = {}
    for u, i, f in zip(*trip):
        out.setdefault(int(u), []).append((int(i), float(f)))
    return {u: sorted(rows) for u, rows in out.items()}


def same_split(ref, mine, name):
    for key in ('train_users', 'test_users', 'items'):
        assert (ref[key] is None) == (mine[key] is None), (name, key)
        assert ref[key] is None or np.array_equal(ref[key], mine[key]), '%s: %s differs' % (name, key)
    assert all(np.array_equal(a, b) for a, b in zip(ref['training'], mine['training'])), name + ': training rows differ'
    for key in ('testset', 'holdout'):
        assert (ref[key] is None) == (mine[key] is None), (name, key)
        if ref[key] is not None:
            assert len(ref[key][0]) == len(mine[key][0]) and user_sets(ref[key]) == user_sets(mine[key]), '%s: %s differs' % (name, key)
            assert (np.diff(ref[key][0]) >= 0).all(), name + ': not sorted by user'


def fixture(name, df, config, custom_order=None):
    ref, data = reference_split(df, config, custom_order)
    cols = dict(users=df['userid'].values.astype(np.int64), items=df['itemid'].values.astype(np.int64),
                feedback=df['rating'].values.astype(np.float64))
    order = None if custom_order is None else df[custom_order].values.astype(np.int64)
    mine = twin.prepare_reference(cols['users'], cols['items'], cols['feedback'], order, config, seed=0)
    same_split(ref, mine, name)
    out = dict(cols, config=np.array(json.dumps(config)), holdout_size=np.int64(ref['holdout_size']))
    if order is not None:
        out['custom_order'] = order
    for key, names in (('training', 'train'), ('testset', 'test'), ('holdout', 'hold')):
        if ref[key] is not None:
            for col, a in zip(('user', 'item', 'fdbk'), ref[key]):
                out['%s_%s' % (names, col)] = a
    for key in ('train_users', 'test_users', 'items'):
        if ref[key] is not None:
            out['index_' + key] = ref[key]
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-18s %6d rows: training %6d, testset %s, holdout %s, %d training / %s test users, %d bytes'
          % (name, len(df), len(ref['training'][0]), None if ref['testset'] is None else len(ref['testset'][0]),
             None if ref['holdout'] is None else len(ref['holdout'][0]), len(ref['train_users']),
             None if ref['test_users'] is None else len(ref['test_users']), os.path.getsize(path)))
    return ref, data


def order_case():
    """Rule 4: an item that occurs only in rows of the test fold, with the lowest rating of all.  Sampling the two worst
    rows of a user BEFORE the unseen item is filtered leaves that user one row; sampling after would leave two."""
    df = raw(seed=11)
    config = dict(test_ratio=0.2, test_fold=5, holdout_size=2, test_sample=-2)
    users = np.sort(df['userid'].unique())
    fold_users = users[round(4 * len(users) * 0.2):]
    long_users = [u for u in fold_users if (df['userid'] == u).sum() >= 6][:12]
    assert len(long_users) >= 8
    extra = pd.DataFrame({'userid': long_users, 'itemid': 99999, 'rating': 0.5})
    df = pd.concat([df, extra]).sample(frac=1, random_state=np.random.RandomState(3)).reset_index(drop=True)
    ref, _ = fixture('prepare_order', df, config)
    sizes = {u: len(rows) for u, rows in user_sets(ref['testset']).items()}
    test_old = ref['test_users']
    short = [u for u, s in sizes.items() if s < 2 and test_old[u] in set(long_users)]
    assert short, 'prepare_order: sampling before and after the filters coincide'
    # every such user had at least two rows of training items to sample from: the other order gives them two rows
    for u in short:
        rows = df[(df['userid'] == test_old[u]) & (df['itemid'] != 99999)]
        assert len(rows) - 2 >= 2
    print('prepare_order: %d users keep one row where sampling after the filters would keep two' % len(short))


def time_reference():
    """`prepare()` of the reference on a larger frame, on this machine (quoted in DESIGN.md §8r with the machine named)"""
    df = raw(n_users=20000, n_items=3000, seed=5)
    data = RecommenderData(df, 'userid', 'itemid', 'rating', seed=0)
    data.verbose = False
    t0 = time.perf_counter()
    quiet(data.prepare)
    print('reference prepare(), state 4 defaults, %d rows x %d users: %.2f s' % (len(df), 20000, time.perf_counter() - t0))


def main():
    df = raw()
    fixture('prepare_s4_default', df, dict(test_ratio=0.2, test_fold=5, holdout_size=3))
    fixture('prepare_s4_fold2', df, dict(test_ratio=0.25, test_fold=2, holdout_size=1))
    fixture('prepare_s4_negative', df, dict(test_ratio=0.2, test_fold=3, holdout_size=2, negative_prediction=True))
    fixture('prepare_s3', df, dict(test_ratio=0.2, test_fold=1, holdout_size=3, warm_start=False))
    ref, _ = fixture('prepare_s2', df, dict(test_ratio=0, holdout_size=5, warm_start=False))
    print('prepare_s2: %d of %d users are too short for the holdout' % (400 - len(np.unique(ref['holdout'][0])), 400))
    fixture('prepare_s1', df, dict(test_ratio=0, holdout_size=0, warm_start=False))
    fixture('prepare_custom_order', raw(seed=9, with_order=True), dict(test_ratio=0.2, test_fold=4, holdout_size=3),
            custom_order='when')
    fixture('prepare_sample_neg4', df, dict(test_ratio=0.2, test_fold=5, holdout_size=3, test_sample=-4))
    order_case()
    if '--time' in sys.argv:
        time_reference()


if __name__ == '__main__':
    main()
