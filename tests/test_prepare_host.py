"""RecommenderArrayData on the host (PrepareNumpyOps): the fixtures made by the reference's own `prepare()`
(tests/golden/make_golden_prepare.py) reproduced exactly, the random modes' properties, configuration errors, events and a
model run.  No GPU."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from numpy_ops import NumpyOps
from polara_amd import ArrayData, PopularityModel, SVDModel
from polara_amd.prepare import PrepareNumpyOps, RecommenderArrayData, mix64
import prepare_reference as twin

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'prepare_*.npz')))
EXPECTED = ['prepare_custom_order', 'prepare_order', 'prepare_s1', 'prepare_s2', 'prepare_s3', 'prepare_s4_default',
            'prepare_s4_fold2', 'prepare_s4_negative', 'prepare_sample_neg4']


class PopNumpyOps(NumpyOps):
    """the two operators PopularityModel needs, on the host: pk_popular_order and pk_popular_topk restated"""

    def popular_order(self, scores):
        s = np.asarray(scores, dtype=np.float64)
        return torch.from_numpy(np.lexsort((np.arange(len(s)), -s)).astype(np.int32))

    def popular_topk(self, T, order, topk, filter_seen):
        order, indptr, indices = np.asarray(order, dtype=np.int64), np.asarray(T.indptr), np.asarray(T.indices)
        out = np.empty((T.shape[0], topk), dtype=np.int64)
        for r in range(T.shape[0]):
            seen = np.isin(order, indices[indptr[r]:indptr[r + 1]]) if filter_seen else np.zeros(len(order), dtype=bool)
            out[r] = np.r_[order[~seen], order[seen]][:topk]
        return torch.from_numpy(out)


def from_fixture(g, ops=None, seed=0):
    config = json.loads(str(g['config']))
    order = g['custom_order'] if 'custom_order' in g.files else None
    return RecommenderArrayData(g['users'], g['items'], g['feedback'], custom_order=order, config=config, seed=seed,
                                ops=ops or PrepareNumpyOps())


def user_sets(trip):
    out = {}
    for u, i, f in zip(*trip):
        out.setdefault(int(u), []).append((int(i), float(f)))
    return {u: sorted(rows) for u, rows in out.items()}


def check_against_fixture(data, g):
    """everything the fixture holds: training rows in order, the three indices, testset and holdout as per-user row sets
    (every row of every user), shapes and holdout_size"""
    tr = data.training
    assert np.array_equal(tr.userid, g['train_user']) and np.array_equal(tr.itemid, g['train_item'])
    assert np.array_equal(tr.feedback, g['train_fdbk'])
    assert np.array_equal(data.index.userid.training.old, g['index_train_users'])
    assert np.array_equal(data.index.userid.training.new, np.arange(len(g['index_train_users'])))
    assert np.array_equal(data.index.itemid.old, g['index_items'])
    assert np.array_equal(data.index.itemid.new, np.arange(len(g['index_items'])))
    assert data.index.feedback is None
    assert (data.n_users, data.n_items) == (len(g['index_train_users']), len(g['index_items']))
    if 'index_test_users' in g.files:
        assert np.array_equal(data.index.userid.test.old, g['index_test_users'])
    else:
        assert data.index.userid.test is None
    for part, name in ((data.test.testset, 'test'), (data.test.holdout, 'hold')):
        if name + '_user' not in g.files:
            assert part is None
            continue
        want = (g[name + '_user'], g[name + '_item'], g[name + '_fdbk'])
        assert len(part.userid) == len(want[0]) and np.array_equal(part.userid, want[0])       # both sorted by user
        assert user_sets(part) == user_sets(want)
    assert data.holdout_size == int(g['holdout_size'])
    if data.test.holdout is not None:
        assert data.get_test_shape() == (len(np.unique(g['hold_user'])), len(g['index_items']))


def same_arrays(a, b):
    """two prepared objects (or twin dicts), array for array"""
    def parts(x):
        if isinstance(x, dict):
            return [x['training'], x['testset'], x['holdout']], [x['train_users'], x['test_users'], x['items']]
        ix = x.index
        return ([x.training, x.test.testset, x.test.holdout],
                [ix.userid.training.old, None if ix.userid.test is None else ix.userid.test.old, ix.itemid.old])
    (ta, ia), (tb, ib) = parts(a), parts(b)
    for p, q in zip(ta, tb):
        assert (p is None) == (q is None)
        if p is not None:
            assert all(np.array_equal(x, y) for x, y in zip(p, q))
    for p, q in zip(ia, ib):
        assert (p is None) == (q is None)
        assert p is None or np.array_equal(p, q)


def test_all_fixtures_are_here():
    assert FIXTURES == EXPECTED


@pytest.mark.parametrize('name', EXPECTED)
def test_fixture_reproduced(name):
    g = load_golden(name)
    data = from_fixture(g)
    check_against_fixture(data, g)
    # the twin gives the same arrays, the order inside a user included (both keep the original order)
    order = g['custom_order'] if 'custom_order' in g.files else None
    same_arrays(data, twin.prepare_reference(g['users'], g['items'], g['feedback'], order, json.loads(str(g['config'])), seed=0))


def test_mix64_is_splitmix64():
    M = 2 ** 64 - 1

    def by_hand(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    zs = [0, 1, 12345, 2 ** 63, M]
    assert by_hand(0) == 0xE220A8397B1DCDAF                    # the first output of splitmix64 seeded with 0
    for f in (mix64, twin.mix64):
        assert [int(x) for x in f(np.array(zs, dtype=np.uint64))] == [by_hand(z) for z in zs]


def test_numpy_ops_match_the_twin():
    rng = np.random.default_rng(3)
    ops = PrepareNumpyOps()
    lens = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025]
    seg = np.r_[0, np.cumsum(lens)].astype(np.int64)
    n = int(seg[-1])
    vals = rng.choice([-1.5, -0.0, 0.0, 5e-324, 2.0], n)
    pos = rng.permutation(n).astype(np.int64) + 2 ** 31 - 100
    for mode in (0, 1, 2, 3, 6, 9):
        hi, lo = ops.split_keys(vals, pos, mode, 5)
        thi, tlo = twin.split_keys(vals, pos, mode, 5)
        assert np.array_equal(hi.view(np.uint64), thi) and np.array_equal(lo.view(np.uint64), tlo)
        for k in (1, 3, 64, 65, 256, 2000):
            assert np.array_equal(ops.segment_select(seg, hi, lo, k), twin.segment_select(seg, thi, tlo, k).astype(bool))
    hi, _ = twin.split_keys(np.array([-2.0, -5e-324, -0.0, 0.0, 5e-324, 1.0]), np.arange(6), 1, 0)
    assert hi[2] == hi[3] and (np.diff(hi.astype(object)) >= 0).all() and len(set(hi.tolist())) == 5


def raw_columns(seed, n_users=120, n_items=60, feedback=True):
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(5000, n_users, replace=False))
    users = np.concatenate([np.full(int(c), u) for u, c in zip(ids, rng.integers(1, 25, n_users))])
    items = np.concatenate([rng.choice(n_items, int(c), replace=False) * 3 + 7 for c in np.bincount(np.searchsorted(ids, users))])
    p = rng.permutation(len(users))
    users, items = users[p], items[p]
    return users, items, (rng.integers(1, 6, len(users)).astype(np.float64) if feedback else None)


@pytest.mark.parametrize('config', [dict(random_holdout=True), dict(permute_tops=True),
                                    dict(permute_tops=True, negative_prediction=True), dict(test_sample=3),
                                    dict(random_holdout=True, warm_start=False, test_ratio=0, holdout_size=2)])
def test_random_modes(config):
    users, items, fb = raw_columns(1)
    cfg = dict(dict(test_ratio=0.25, test_fold=2, holdout_size=3), **config)
    a = RecommenderArrayData(users, items, fb, config=cfg, seed=4, ops=PrepareNumpyOps())
    same_arrays(a, RecommenderArrayData(users, items, fb, config=cfg, seed=4, ops=PrepareNumpyOps()))
    same_arrays(a, twin.prepare_reference(users, items, fb, None, cfg, seed=4))
    b = RecommenderArrayData(users, items, fb, config=cfg, seed=5, ops=PrepareNumpyOps())
    differs = not np.array_equal(a.test.holdout.itemid, b.test.holdout.itemid)
    if 'test_sample' in config:
        differs = not np.array_equal(a.test.testset.itemid, b.test.testset.itemid)
    assert differs and a.seed_used == 4
    # rows come from the right user, and from the fold; holdout rows have the user's top values unless drawn at random
    pairs = set(zip(users.tolist(), items.tolist()))
    uid = a.index.userid.test if a.index.userid.test is not None else a.index.userid.training
    hold_users = uid.old[a.test.holdout.userid]
    assert all((u, i) in pairs for u, i in zip(hold_users.tolist(), a.index.itemid.old[a.test.holdout.itemid].tolist()))
    if cfg['test_ratio']:
        distinct = np.unique(users)
        code = np.searchsorted(distinct, hold_users)
        assert code.min() >= round(len(distinct) * 0.25) and code.max() < round(2 * len(distinct) * 0.25)
    if config.get('permute_tops'):
        fb_of = {(u, i): f for u, i, f in zip(users.tolist(), items.tolist(), fb.tolist())}
        sign = -1 if config.get('negative_prediction') else 1
        for u in np.unique(hold_users):
            mine = sorted(sign * f for (uu, _), f in fb_of.items() if uu == u)[-3:]
            assert sorted(sign * f for f in a.test.holdout.feedback[hold_users == u]) == mine
    assert (np.unique(a.test.holdout.userid, return_counts=True)[1] == cfg['holdout_size']).all()


def test_random_selection_counts_and_row_permutation():
    """before the filters: min(holdout_size, len) rows per user; a permutation of the rows with the same positions p gives the
    same set of rows (the draw of a row depends on (seed, p) alone)"""
    ops = PrepareNumpyOps()
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 9, 50)
    seg = np.r_[0, np.cumsum(lens)].astype(np.int64)
    n = int(seg[-1])
    pos = rng.permutation(n).astype(np.int64)
    hi, lo = ops.split_keys(None, pos, 6, 9)
    flags = ops.segment_select(seg, hi, lo, 3)
    assert np.array_equal(np.add.reduceat(np.r_[flags, False].astype(int), seg[:-1])[lens > 0], np.minimum(3, lens)[lens > 0])
    chosen = set(pos[flags].tolist())
    shuffled = np.concatenate([b + rng.permutation(e - b) for b, e in zip(seg[:-1], seg[1:])]).astype(np.int64)
    hi2, lo2 = ops.split_keys(None, pos[shuffled], 6, 9)
    assert set(pos[shuffled][ops.segment_select(seg, hi2, lo2, 3)].tolist()) == chosen
    # no feedback: the holdout is drawn at random
    users, items, _ = raw_columns(3, feedback=False)
    d = RecommenderArrayData(users, items, None, config=dict(holdout_size=2, test_ratio=0.5, test_fold=1), seed=1, ops=ops)
    same_arrays(d, twin.prepare_reference(users, items, None, None, dict(holdout_size=2, test_ratio=0.5, test_fold=1), seed=1))
    assert (d.training.feedback == 1).all()
    d2 = RecommenderArrayData(users, items, None, config=dict(holdout_size=2, test_ratio=0.5, test_fold=1), ops=ops)
    d2.update()
    assert isinstance(d2.seed_used, int)


def test_configuration_errors():
    users, items, fb = raw_columns(4)
    new = lambda **cfg: RecommenderArrayData(users, items, fb, config=cfg, seed=0, ops=PrepareNumpyOps())
    with pytest.raises(ValueError, match='Both holdout_size and test_ratio must be positive when warm_start is set to True'):
        new(test_ratio=0).prepare()
    with pytest.raises(ValueError, match='Both holdout_size and test_ratio must be positive'):
        new(holdout_size=0).prepare()
    with pytest.raises(ValueError, match='Test fold value cannot be greater than 5.0'):
        new(test_fold=6).prepare()
    with pytest.raises(AssertionError, match='test_ratio'):
        new(test_ratio=1.0, test_fold=1).prepare()
    with pytest.raises(NotImplementedError, match='holdout_size'):
        new(holdout_size=0.3).prepare()
    with pytest.raises(ValueError, match='test_ratio cannot be nonzero when holdout_size is 0 and warm_start is set to False'):
        # (the reference's state 11: its own validation, restated here, refuses the configuration before the state is reached)
        new(holdout_size=0, warm_start=False, test_ratio=0.2).training
    with pytest.raises(NotImplementedError, match='test_sample'):
        new(test_sample=0.5).prepare()
    d = new()
    with pytest.raises(NotImplementedError, match='ensure_consistency'):
        d.ensure_consistency = False
    with pytest.raises(NotImplementedError, match='build_index'):
        d.build_index = False
    assert not hasattr(d, 'get_entity_index')
    with pytest.raises(NotImplementedError, match='Data has duplicate values'):
        RecommenderArrayData(np.r_[users, users[:1]], np.r_[items, items[:1]], np.r_[fb, 1.0], ops=PrepareNumpyOps())
    with pytest.raises(ValueError, match='finite'):
        RecommenderArrayData(users, items, np.where(np.arange(len(fb)) == 3, np.nan, fb), ops=PrepareNumpyOps())
    assert RecommenderArrayData.default_configuration() == dict(
        test_ratio=0.2, test_fold=5, warm_start=True, holdout_size=3, test_sample=None, permute_tops=False,
        random_holdout=False, negative_prediction=False, shuffle_data=False)
    assert d.get_configuration() == RecommenderArrayData.default_configuration()


def test_events_lazy_update_and_models():
    users, items, fb = raw_columns(6, n_users=200)
    data = RecommenderArrayData(users, items, fb, config=dict(test_ratio=0.25, test_fold=4), seed=0, ops=PrepareNumpyOps())
    m = SVDModel(data, ops=NumpyOps())
    m.verbose = False
    m.rank, m.topk = 5, 5
    m.build()                                                   # lazy: the first access prepares
    assert data._state == 4 and m._is_ready
    recs = m.recommendations
    assert m._recommendations is not None
    calls = []

    class Listener:
        def changed(self):
            calls.append('change')

        def updated(self):
            calls.append('update')
    listener = Listener()
    data.subscribe(data.on_change_event, listener.changed)
    data.subscribe(data.on_update_event, listener.updated)
    data.prepare()                                              # nothing changed: nothing happens
    assert calls == [] and m._is_ready and m._recommendations is not None
    training = data.training
    data.holdout_size = 2                                       # test side only
    data.shuffle_data = False                                   # (the same value: no change)
    assert calls == []
    assert data.test.holdout is not None and calls == ['update']
    assert m._is_ready and m._recommendations is None           # the model stays, its lists go
    assert data.training is training                            # the training part was left alone
    assert (np.bincount(data.test.holdout.userid) == 2).all() and data.holdout_size == 2
    fresh = RecommenderArrayData(users, items, fb, config=dict(test_ratio=0.25, test_fold=4, holdout_size=2), seed=0,
                                 ops=PrepareNumpyOps())
    same_arrays(data, fresh)                                    # a test-side update equals a fresh object
    assert m.recommendations.shape == (data.get_test_shape()[0], 5)
    data.test_sample = -3
    data.update()
    assert calls == ['update', 'update'] and data.training is training
    data.test_fold = 3                                          # another fold: everything anew
    data.update()
    assert calls == ['update', 'update', 'change'] and not m._is_ready and data.training is not training
    data.set_configuration(dict(test_sample=None, seed=7))      # the seed is part of the configuration: a full update
    assert data.test is not None and calls[-1] == 'change' and len(calls) == 4
    data.prepare_training_only()
    assert data._state == 1 and data.test.holdout is None and data.test.testset is None and calls[-1] == 'change'
    assert len(data.training.userid) == len(users) and data.n_users == 200 and data.get_configuration()['holdout_size'] == 0
    assert np.array_equal(data.external_users(data.training.userid), users)
    assert np.array_equal(data.external_items(data.training.itemid), items)
    assert recs.shape[1] == 5


@pytest.mark.parametrize('config', [dict(test_ratio=0.25, test_fold=4), dict(test_ratio=0.25, test_fold=1, warm_start=False),
                                    dict(test_ratio=0, warm_start=False, holdout_size=1)])
def test_models_on_prepared_data(config):
    """SVDModel and PopularityModel give on a prepared object what they give on an ArrayData fed the same arrays"""
    users, items, fb = raw_columns(8, n_users=200)
    data = RecommenderArrayData(users, items, fb, config=config, seed=0, ops=PrepareNumpyOps())
    plain = ArrayData(data.training, n_users=data.n_users, n_items=data.n_items, test=data.test.testset,
                      holdout=data.test.holdout, warm_start=data.warm_start)
    assert plain.holdout_size == data.holdout_size
    for cls in (SVDModel, PopularityModel):
        lists = []
        for d in (data, plain):
            m = cls(d, ops=PopNumpyOps())
            m.verbose = False
            m.topk = 5
            if cls is SVDModel:
                m.rank = 6
            m.build()
            lists.append((m.get_recommendations(), m.evaluate('hits')))
        assert np.array_equal(lists[0][0], lists[1][0]) and lists[0][1] == lists[1][1]
        assert lists[0][0].shape[0] == data.get_test_shape()[0] > 0


def _side_by_side():
    import contextlib
    import io
    import warnings
    warnings.filterwarnings('ignore')
    for p in ('_lightfm_shim', '_sksparse_shim', '_numba_shim'):
        sys.path.insert(0, os.path.join(HERE, 'golden', p))
    sys.path.insert(0, REF)
    import pandas as pd
    from polara.recommender.data import RecommenderData
    users, items, fb = raw_columns(21, n_users=150)
    df = pd.DataFrame({'userid': users, 'itemid': items, 'rating': fb})
    for config in (dict(test_ratio=0.2, test_fold=2, holdout_size=2), dict(test_ratio=0.25, test_fold=4, holdout_size=1, negative_prediction=True),
                   dict(test_ratio=0.2, test_fold=5, holdout_size=3, warm_start=False), dict(test_ratio=0, holdout_size=4, warm_start=False),
                   dict(test_ratio=0, holdout_size=0, warm_start=False), dict(test_ratio=0.2, test_fold=1, holdout_size=2, test_sample=-3)):
        ref = RecommenderData(df, 'userid', 'itemid', 'rating', seed=0)
        ref.verbose = False
        ref.verify_sessions_length_distribution = False
        for k, v in config.items():
            setattr(ref, k, v)
        with contextlib.redirect_stdout(io.StringIO()):
            ref.prepare()
        ours = RecommenderArrayData(users, items, fb, config=config, seed=0, ops=PrepareNumpyOps())
        assert np.array_equal(ours.training.userid, ref.training['userid'].values), config
        assert np.array_equal(ours.training.itemid, ref.training['itemid'].values), config
        assert np.array_equal(ours.training.feedback, ref.training['rating'].values), config
        assert np.array_equal(ours.index.userid.training.old, ref.index.userid.training['old'].values), config
        assert np.array_equal(ours.index.itemid.old, ref.index.itemid['old'].values), config
        assert (ours.index.userid.test is None) == (ref.index.userid.test is None)
        if ref.index.userid.test is not None:
            assert np.array_equal(ours.index.userid.test.old, ref.index.userid.test['old'].values), config
        for mine, theirs in ((ours.test.testset, ref.test.testset), (ours.test.holdout, ref.test.holdout)):
            assert (mine is None) == (theirs is None), config
            if mine is not None:
                want = tuple(theirs[c].values for c in ('userid', 'itemid', 'rating'))
                assert np.array_equal(mine.userid, want[0]) and user_sets(mine) == user_sets(want), config
    print('SIDE_BY_SIDE_OK')


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'polara')), reason='the reference is not on this machine')
def test_side_by_side_with_the_reference():
    """a fresh random matrix through the reference's own prepare() and ours, in a child process (the reference pulls pandas
    and its own `polara` package into the interpreter)"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE]))
    r = subprocess.run([sys.executable, '-c', 'import test_prepare_host as t; t._side_by_side()'], capture_output=True, text=True,
                       env=env, cwd=HERE)
    assert r.returncode == 0 and 'SIDE_BY_SIDE_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
