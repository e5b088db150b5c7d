"""Item-to-item (CooccurrenceModel) and most-popular (PopularityModel) on the device: C against the reference's matrix,
the lists against the reference's (tie-aware) and against the restatement of tests/i2i_reference.py (exactly, under
the total order class / score / item), seeded random shapes, and the model lifecycle."""
import numpy as np
import pytest

import i2i_reference as ref
from conftest import GoldenData, load_golden

pytestmark = pytest.mark.gpu

I2I_FIXTURES = ['i2i_sparse', 'i2i_nofilter', 'i2i_warm', 'i2i_implicit', 'i2i_dense', 'i2i_nondyadic']
MP_FIXTURES = ['mp_count', 'mp_feedback']


def _model(g, hip_ops):
    from polara_amd.models import CooccurrenceModel, PopularityModel
    data = GoldenData(g)
    data.warm_start = bool(g['warm_start'])
    if str(g['model']) == 'MP':
        m = PopularityModel(data, ops=hip_ops)
        m.by_feedback_value = bool(g['by_feedback_value'])
    else:
        m = CooccurrenceModel(data, ops=hip_ops)
        m.implicit = bool(g['implicit'])
        m.dense_output = bool(g['dense_output'])
    m.verbose = False
    m.topk = int(g['topk'])
    m.filter_seen = bool(g['filter_seen'])
    return m


@pytest.mark.parametrize('name', I2I_FIXTURES)
def test_device_i2i_matrix_equals_the_reference(name, hip_ops):
    g = load_golden(name)
    m = _model(g, hip_ops)
    m.build()
    n = int(g['train_shape'][1])
    C = m.i2i_matrix.double().cpu().numpy()
    assert C.shape == (n, -(-n // 8) * 8) and not C[:, n:].any()
    R = np.zeros((n, n))
    R[g['c_row'], g['c_col']] = g['c_val']
    if name == 'i2i_nondyadic':
        assert m.i2i_dtype == 'float64'
        assert np.allclose(C[:, :n], R, rtol=1e-12, atol=1e-12)
    else:
        assert m.i2i_dtype == 'float32'
        assert np.array_equal(C[:, :n], R)
    assert len(m.training_time) == 1


@pytest.mark.parametrize('name', I2I_FIXTURES + MP_FIXTURES)
def test_lists_match_the_reference_and_the_restatement(name, hip_ops):
    g = load_golden(name)
    m = _model(g, hip_ops)
    recs = m.recommendations
    scores, cls, lists = ref.fixture_lists(g)
    assert recs.shape == g['recs'].shape and recs.dtype == np.int64
    if name == 'i2i_nondyadic':                 # fp64 sums in another order: equal scores may differ in the last bits
        assert ref.tie_aware_mismatches(recs, g['recs'], scores, cls, tol=1e-12) == []
        assert ref.tie_aware_mismatches(recs, lists, scores, cls, tol=1e-12) == []
    else:
        assert ref.tie_aware_mismatches(recs, g['recs'], scores, cls) == []
        assert np.array_equal(recs, lists)


def _random_case(rng, n_users, n_items, per_user, negative=False, step=1.0, heavy=0):
    """(training COO, test CSR arrays, test triplet) with empty test rows, rows holding only zero-feedback entries and
    `heavy` users that hold most of the catalogue."""
    tr_u, tr_i, tr_v = [], [], []
    for u in range(n_users):
        k = min(n_items, rng.integers(1, per_user + 1) if u >= heavy else int(0.8 * n_items))
        items = rng.choice(n_items, k, replace=False)
        vals = rng.integers(1, 6, k) * step
        if negative:
            vals = np.where(rng.random(k) < 0.25, -vals, vals)
        tr_u.append(np.full(k, u))
        tr_i.append(items)
        tr_v.append(vals)
    idx = np.stack([np.concatenate(tr_u), np.concatenate(tr_i)], 1).astype(np.int64)
    val = np.concatenate(tr_v).astype(np.float64)
    n_test = max(4, n_users // 3)
    te_u, te_i, te_v = [], [], []
    for r in range(n_test):
        kind = r % 7
        if kind == 0:
            continue                                           # empty row
        k = min(n_items, rng.integers(1, per_user + 1) if r >= heavy else int(0.6 * n_items))
        items = np.sort(rng.choice(n_items, k, replace=False))
        vals = rng.integers(1, 6, k) * step
        if kind == 1:
            vals = np.zeros(k)                                 # only zero-feedback entries: seen, no score
        elif negative:
            vals = np.where(rng.random(k) < 0.25, -vals, vals)
        te_u.append(np.full(k, r))
        te_i.append(items)
        te_v.append(vals)
    tu, ti, tv = (np.concatenate(x) for x in (te_u, te_i, te_v))
    return idx, val, (tu.astype(np.int64), ti.astype(np.int64), tv.astype(np.float64)), (n_test, n_items)


CASES = [  # (n_users, n_items, per_user, topk, negative, step, heavy)
    (60, 300, 20, 1, False, 1.0, 0),
    (80, 2048, 40, 10, True, 1.0, 0),
    (50, 2048, 30, 100, False, 0.1, 0),
    (40, 5000, 60, 1024, True, 1.0, 2),
    (70, 4500, 15, 10, False, 1.0, 3),
    (30, 6200, 25, 100, False, 0.3, 1),
    (40, 1030, 8, 1024, False, 1.0, 0),
]


@pytest.mark.parametrize('case', range(len(CASES)))
def test_seeded_shapes_against_the_restatement(case, hip_ops):
    from polara_amd import i2i
    n_users, n_items, per_user, topk, negative, step, heavy = CASES[case]
    rng = np.random.default_rng(1000 + case)
    idx, val, test, tshape = _random_case(rng, n_users, n_items, per_user, negative, step, heavy)
    A = hip_ops.csr_from_coo(idx[:, 0], idx[:, 1], val, (n_users, n_items))
    C, dtype = hip_ops.i2i_build(A)
    Cr = ref.i2i_matrix(ref.training_matrix(idx, val, (n_users, n_items)))
    exact = np.array_equal(Cr.astype(np.float32).astype(np.float64), Cr)
    assert dtype == ('float32' if exact else 'float64')
    Cd = C.double().cpu().numpy()
    assert C.shape[1] == i2i.leading_dim(n_items) and not Cd[:, n_items:].any()
    if step == 1.0:
        assert np.array_equal(Cd[:, :n_items], Cr)
    else:
        assert np.allclose(Cd[:, :n_items], Cr, rtol=1e-12, atol=1e-12)
    T, seen = ref.test_matrix(test, tshape)
    scores = ref.i2i_scores(Cr, T)
    order = np.lexsort((test[1], test[0]))
    tu, ti, tv = (x[order] for x in test)
    indptr = np.r_[0, np.cumsum(np.bincount(tu, minlength=tshape[0]))]
    Td = hip_ops.csr(indptr, ti, tv, tshape)
    for sparse in (True, False):
        for filter_seen in (True, False):
            want = ref.select(scores, seen, topk, filter_seen, sparse)
            got, got_s = hip_ops.i2i_topk(Td, C, n_items, topk, filter_seen, sparse, want_scores=True)
            got, got_s = got.cpu().numpy(), got_s.cpu().numpy()
            live = got >= 0
            ref_s = np.take_along_axis(scores, np.maximum(got, 0), 1)
            if step == 1.0:
                assert np.array_equal(got, want), (sparse, filter_seen)
                assert np.array_equal(got_s[live], ref_s[live])
            else:
                assert np.allclose(got_s[live], ref_s[live], rtol=1e-12, atol=1e-12)
                cls = ref.classes(scores, seen, filter_seen, sparse)
                assert ref.tie_aware_mismatches(got, want, scores, cls, tol=1e-12) == [], (sparse, filter_seen)
            if sparse:
                assert (got[0] == -1).all() and (got[1] == -1).all()     # the empty row and the zero-feedback row
    if case == 3:
        with pytest.raises(Exception, match='1024'):
            hip_ops.i2i_topk(Td, C, n_items, 1025, True, True)


def test_popularity_with_tied_counts(hip_ops):
    from polara_amd.data import ArrayData
    from polara_amd.models import PopularityModel
    rng = np.random.default_rng(7)
    n_users, n_items = 500, 3000
    u = rng.integers(0, n_users, 6000)
    i = rng.integers(0, n_items // 3, 6000)                    # a third of the catalogue is ever rated: ties at 0 too
    uniq = np.unique(np.stack([u, i], 1), axis=0)
    u, i = uniq[:, 0], uniq[:, 1]
    v = rng.integers(1, 6, len(u)).astype(np.float64)
    hold = (np.arange(n_users), rng.integers(0, n_items, n_users), np.ones(n_users))
    data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=hold, warm_start=False)
    idx = np.stack([u, i], 1)
    for by_value in (False, True):
        for topk in (1, 10, 2999):
            for fs in (True, False):
                m = PopularityModel(data, ops=hip_ops)
                m.verbose, m.by_feedback_value, m.topk, m.filter_seen = False, by_value, topk, fs
                recs = m.recommendations
                s = ref.popularity_scores(idx, v, n_items, by_value)
                assert len(np.unique(s)) < n_items
                (tu, ti, tf), tshape, _ = m._get_test_data()
                _, seen = ref.test_matrix((tu, ti, tf), tshape)
                want = ref.select(np.repeat(s[None], tshape[0], 0), seen, topk, fs, False)
                assert np.array_equal(recs, want), (by_value, topk, fs)
    with pytest.raises(ValueError, match='out of bounds'):
        m.topk = n_items + 1
        m.get_recommendations()


def test_lifecycle(hip_ops):
    from polara_amd.data import ArrayData
    from polara_amd.models import CooccurrenceModel
    rng = np.random.default_rng(11)
    n_users, n_items = 300, 2500
    u = np.repeat(np.arange(n_users), 4)
    i = rng.integers(0, n_items, len(u))
    uniq = np.unique(np.stack([u, i], 1), axis=0)
    u, i = uniq[:, 0], uniq[:, 1]
    v = rng.integers(1, 6, len(u)).astype(np.float64)
    hold = (np.arange(n_users), rng.integers(0, n_items, n_users), np.ones(n_users))
    data = ArrayData((u, i, v), n_users=n_users, n_items=n_items, holdout=hold, warm_start=False)
    m = CooccurrenceModel(data, ops=hip_ops)
    m.verbose = False
    m.topk = 50
    recs = m.recommendations
    assert (recs == -1).any() and len(m.training_time) == 1 and m.i2i_dtype == 'float32'
    m.topk = 20                                                # shrinking keeps the cached lists
    assert m.recommendations is recs
    m.topk = 60                                                # growing re-scores, no rebuild
    assert np.array_equal(m.recommendations[:, :50], recs) and len(m.training_time) == 1
    m.dense_output = True                                      # another branch: new lists, same model
    dense = m.recommendations
    assert not (dense == -1).any() and len(m.training_time) == 1
    data.set_training_data((u, i, v * 2))                      # a data change: a new model
    assert m._i2i is None and not m._is_ready
    m.recommendations
    assert len(m.training_time) == 2 and m.i2i_dtype == 'float32'
    # show_recommendations (sparse and dense) against the restatement
    (tu, ti, tf), tshape, _ = m._get_test_data()
    Cr = ref.i2i_matrix(ref.training_matrix(np.stack([u, i], 1), v * 2, (n_users, n_items)))
    T, seen = ref.test_matrix((tu, ti, tf), tshape)
    scores = ref.i2i_scores(Cr, T)
    for dense_output in (False, True):
        m.dense_output = dense_output
        top, seen_items = m.show_recommendations(5, topk=10)
        want = ref.select(scores[5:6], seen[5:6], 10, True, not dense_output)[0]
        assert np.array_equal(top, want) and set(seen_items) == set(ti[tu == 5])
    m.dense_output = False
    res = m.evaluate(topk=10)
    assert res is not None
    m.topk = 10
    lists, list_scores = m.recommend_with_scores()
    assert lists.shape == list_scores.shape == (tshape[0], 10) and np.array_equal(lists, m.get_recommendations())
    assert np.array_equal(list_scores[lists >= 0], np.take_along_axis(scores, np.maximum(lists, 0), 1)[lists >= 0])
