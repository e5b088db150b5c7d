"""Item cold start, host side (no GPU): the NumPy/SciPy restatement (tests/coldstart_reference.py) against the reference's
own fixtures (tests/golden/coldstart_*.npz from tests/golden/make_golden_coldstart.py), the two data classes, our
`stack_features`, rank truncation, cache invalidation, the memory guard, MP(cs), and the models' orchestration on a CPU
double of the device operators."""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

import coldstart_reference as ref
from conftest import load_golden
from test_hybrid_host import HybridNumpyOps

FACTOR_FIXTURES = ['coldstart_svd', 'coldstart_svd_scaled', 'coldstart_hybrid', 'coldstart_hybrid_scaled', 'coldstart_repr',
                   'coldstart_odd_features']
# The reference's evaluate() numbers that are compared: the hit counts, the coverage, and MAP and ARHR of the ranking
# family.  Precision, recall, miss rate, fallout, specificity, nDCG and nDCL go through the reference's `safe_divide`
# (`np.divide(a, b, where=mask)` with no `out=`, polara/recommender/evaluation.py:18-20): the entries outside the mask are
# whatever the allocator handed back, so the reference's values of THOSE fields depend on the allocation history of the
# process; the fixtures keep them as a record of what the reference printed, not as a contract.
EVAL_KEYS = ('eval_Hits_true_positive', 'eval_Hits_false_positive', 'eval_Hits_false_negative', 'eval_Experience_coverage',
             'eval_Ranking_map', 'eval_Ranking_arhr')


class ColdStartNumpyOps(HybridNumpyOps):
    """The CPU double plus the cold-start query operator (same layout: even leading dimension, zero padding)."""

    def coldstart_queries(self, F, W, G):
        E = np.asarray(F.m @ W.numpy()) @ G.numpy()
        n, rank = E.shape
        block = torch.zeros(n, rank + (rank & 1), dtype=torch.float64)
        block[:, :rank] = torch.from_numpy(E)
        return block[:, :rank]


def golden_data(g):
    from polara_amd.data import ItemColdStartArrayData, ItemColdStartSimilarityArrayData
    idx = g['train_idx']
    shp = tuple(int(x) for x in g['train_shape'])
    args = ((idx[:, 0], idx[:, 1], g['train_val']), (g['hold_user'], g['hold_cold'], g['hold_fdbk']),
            ref.one_hot(g, 'ft'), ref.one_hot(g, 'fc'))
    kw = dict(n_users=shp[0], n_items=shp[1], representative_users=g['repr_users'] if 'repr_users' in g else None)
    if 'rel_row' in g:
        S = sps.csr_matrix((g['rel_val'], (g['rel_row'], g['rel_col'])), shape=(shp[1], shp[1]))
        return ItemColdStartSimilarityArrayData(*args, relations_matrices={'itemid': S, 'userid': None},
                                                relations_indices={'itemid': None, 'userid': None}, **kw)
    return ItemColdStartArrayData(*args, **kw)


MODELS = {'PureSVD(cs)': 'SVDModelItemColdStart', 'PureSVD(cs)-s': 'ScaledSVDItemColdStart',
          'HybridSVD(cs)': 'HybridSVDItemColdStart', 'HybridSVD(cs)-s': 'ScaledHybridSVDItemColdStart'}


def model_for(g, ops, data=None):
    from polara_amd import coldstart
    m = getattr(coldstart, MODELS[str(g['model'])])(golden_data(g) if data is None else data, ops=ops)
    m.verbose = False
    m.rank, m.topk = int(g['rank']), int(g['topk'])
    if 'features_weight' in g:
        m.features_weight = float(g['features_weight'])
    return m


def check_model_against_fixture(m, g, tol_sigma=1e-9, tol_vec=1e-8, tol_scores=1e-9):
    """what the issue asks of every model: sigma, W and projectors up to column signs, scores, lists, lists after rank = 5,
    evaluate() — shared with the device tests"""
    m.build()
    itemid = m.data.fields.itemid
    assert m.method == str(g['model']) and m.filter_seen is False and m._prediction_key == 'itemid_cold'
    assert np.allclose(m.factors['singular_values'], g['sigma'], rtol=tol_sigma, atol=0)
    W = m.factors[f'{itemid}_features']
    assert W.shape == g['W'].shape and ref.same_up_to_sign(W, g['W'], tol_vec)
    assert ref.same_up_to_sign(m.factors[m.data.fields.userid], g['U'], tol_vec)
    if 'vr' in g:
        vl, vr = m.get_item_projector()
        assert ref.same_up_to_sign(vl, g['vl'], tol_vec) and ref.same_up_to_sign(vr, g['vr'], tol_vec)
    else:
        assert ref.same_up_to_sign(m.factors[itemid], g['V'], tol_vec)
    n = g['scores'].shape[0]
    s = m.slice_recommendations(None, 0, n)
    assert np.abs(s - g['scores']).max() <= tol_scores * np.abs(g['scores']).max()
    recs = m.get_recommendations()
    assert recs.dtype == np.int64 and np.array_equal(recs, g['recs'])
    scores = {type(x).__name__: x for x in m.evaluate('all')}
    for key in EVAL_KEYS:
        _, family, field = key.split('_', 2)
        assert np.isclose(getattr(scores[family], field), float(g[key]), rtol=1e-12, atol=0), key
    builds = len(m.training_time)
    m.rank = 5
    assert m._is_ready and m._item_features_transform_helper.shape == (5, 5)
    assert np.array_equal(m.get_recommendations(), g['recs_rank5'])
    assert len(m.training_time) == builds == int(g['builds_after_rank5'])


@pytest.mark.parametrize('name', FACTOR_FIXTURES)
def test_restatement_matches_the_reference(name):
    g = load_golden(name)
    r = ref.fixture_model(g)
    assert np.allclose(r['sigma'], g['sigma'], rtol=1e-10, atol=0)
    assert ref.same_up_to_sign(r['W'], g['W'], 1e-8) and ref.same_up_to_sign(r['U'], g['U'], 1e-8)
    n = g['scores'].shape[0]
    assert np.abs(r['scores'][:n] - g['scores']).max() <= 1e-9 * np.abs(g['scores']).max()
    # (column signs are free: column j of W flips row and column j of G)
    assert np.allclose(np.abs(r['G5']), np.abs(g['G_rank5']), rtol=1e-7, atol=1e-9 * np.abs(g['G_rank5']).max())
    assert np.array_equal(r['lists'], g['recs']) and np.array_equal(r['lists5'], g['recs_rank5'])
    assert float(g['min_rel_gap']) >= 1e-6 and float(g['cond_gram']) <= 1e6


def test_column_signs_cancel():
    g = load_golden('coldstart_svd')
    Ft, Fc = ref.one_hot(g, 'ft'), ref.one_hot(g, 'fc')
    flip = np.where(np.arange(int(g['rank'])) % 2, -1.0, 1.0)
    W, G = ref.embeddings(Ft, g['V'])
    W2, G2 = ref.embeddings(Ft, g['V'] * flip)
    a = ref.scores(Fc, W, G, g['U'], g['sigma'])
    b = ref.scores(Fc, W2, G2, g['U'] * flip, g['sigma'])
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()


@pytest.mark.parametrize('name', FACTOR_FIXTURES)
def test_models_on_the_cpu_double(name):
    g = load_golden(name)
    check_model_against_fixture(model_for(g, ColdStartNumpyOps()), g)


def test_representative_users_do_not_restrict_the_factor_models():
    a, b = load_golden('coldstart_svd'), load_golden('coldstart_repr')
    assert 'repr_users' in b and len(b['repr_users']) == 100 and 'repr_users' not in a
    assert np.array_equal(a['recs'], b['recs'])
    assert not np.isin(b['recs'], b['repr_users']).all()


def test_odd_features_through_the_data_object():
    """the fixture's RAW inputs (cold items with only an unknown label, with no label, with known and unknown labels) through
    ItemColdStartArrayData: the first two are dropped and the rest renumbered as the reference does"""
    from polara_amd.data import ItemColdStartArrayData
    g = load_golden('coldstart_odd_features')
    idx = g['train_idx']
    shp = tuple(int(x) for x in g['train_shape'])

    def rows(ptr, lab):
        return [lab[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)]
    nl = int(g['raw_n_labels'])
    from polara_amd.data import one_hot_csr
    data = ItemColdStartArrayData((idx[:, 0], idx[:, 1], g['train_val']), (g['raw_hold_user'], g['raw_hold_cold'], g['raw_hold_fdbk']),
                                  one_hot_csr(rows(g['raw_train_ptr'], g['raw_train_lab']), n_labels=nl),
                                  one_hot_csr(rows(g['raw_cold_ptr'], g['raw_cold_lab']), n_labels=nl),
                                  n_users=shp[0], n_items=shp[1])
    assert data.n_cold_items == int(g['n_cold']) == len(g['raw_cold_old']) - 2
    assert np.array_equal(g['raw_cold_old'][data.cold_items_kept], g['cold_old'])
    u, c, f = data.test.holdout
    assert np.array_equal(c, g['hold_cold'])          # sorted by cold item; the order inside an item is the sort's own
    o1, o2 = np.lexsort((u, c)), np.lexsort((g['hold_user'], g['hold_cold']))
    assert np.array_equal(u[o1], g['hold_user'][o2]) and np.array_equal(f[o1], g['hold_fdbk'][o2])
    assert data.holdout_size == -1
    m = model_for(g, ColdStartNumpyOps(), data=data)
    m.build()
    # the item with known AND unknown labels keeps only its known ones: as many entries as the reference's matrix
    F = m._cold_one_hot()
    assert F.shape == tuple(int(x) for x in g['fc_shape']) and F.nnz == len(g['fc_row'])
    assert np.array_equal(m.get_recommendations(), g['recs'])


def test_empty_query_rows_give_zero_scores():
    g = load_golden('coldstart_svd')
    data = golden_data(g)
    m = model_for(g, ColdStartNumpyOps(), data=data)
    m.build()
    W, G = m._features_device()
    E = m.ops.coldstart_queries(m.ops.csr([0, 0, 2, 2], [1, 3], [1.0, 1.0], (3, W.shape[0])), W, G)
    assert E.shape == (3, int(g['rank'])) and float(E[0].abs().max()) == 0 and float(E[2].abs().max()) == 0 and float(E[1].abs().max()) > 0
    from polara_amd import scoring
    image, order = m._user_factors_device()
    idx, s = scoring.recommend_dense(m.ops, image, E, 5, return_scores=True)
    assert float(s[0].abs().max()) == 0 and float(s[2].abs().max()) == 0
    full = E[1].numpy() @ image.V.numpy().T
    assert np.array_equal(idx[1].numpy(), np.lexsort((np.arange(len(full)), -full))[:5])


def test_data_classes():
    from polara_amd.data import ItemColdStartArrayData, ItemColdStartSimilarityArrayData, one_hot_csr
    tr = (np.array([0, 1, 2, 2]), np.array([0, 1, 0, 2]), np.ones(4))
    hold = (np.array([2, 0, 1, 0]), np.array([1, 0, 1, 2]), np.array([5., 4., 3., 2.]))
    with pytest.raises(ValueError):       # the two matrices must share one label space
        ItemColdStartArrayData(tr, hold, [[0], [1], [0, 1]], [[1], [0, 2], [3]], n_users=3, n_items=3)
    d = ItemColdStartArrayData(tr, hold, one_hot_csr([[0], [1], [0, 1]], n_labels=4), [[1], [0, 2], [3]], n_users=3, n_items=3,
                               representative_users=[2, 0])
    assert d.n_cold_items == 2 and np.array_equal(d.cold_items_kept, [0, 1])        # cold item 2 has only label 3: unknown
    u, c, f = d.test.holdout
    assert np.array_equal(c, [0, 1, 1]) and np.array_equal(u, [0, 2, 1]) and np.array_equal(f, [4., 5., 3.])
    assert np.array_equal(d.representative_users, [0, 2]) and d.holdout_size == -1 and d.test.testset is None
    assert d.get_test_shape() == (2, 3)
    with pytest.raises(NotImplementedError):
        d.holdout_size = 3
    with pytest.raises(ValueError):
        ItemColdStartArrayData(tr, (np.array([7]), np.array([0]), np.ones(1)), one_hot_csr([[0], [1], [0, 1]], n_labels=4),
                               [[1], [0, 2], [3]], n_users=3, n_items=3)
    seen = []

    class Sub:
        def hit(self):
            seen.append(1)
    s = Sub()
    d.subscribe(d.on_update_event, s.hit)
    d.set_test_data(holdout=(np.array([1]), np.array([0]), np.ones(1)))
    assert seen == [1] and d.n_cold_items == 2 and len(d.test.holdout.userid) == 1
    S = sps.identity(3, format='csr')
    ds = ItemColdStartSimilarityArrayData(tr, hold, one_hot_csr([[0], [1], [0, 1]], n_labels=4), [[1], [0, 2], [3]], n_users=3,
                                          n_items=3, relations_matrices={'itemid': S, 'userid': None},
                                          relations_indices={'itemid': None, 'userid': None})
    assert ds.n_cold_items == 2 and ds.item_relations.shape == (3, 3) and ds.user_relations is None


def test_stack_features_follows_the_reference_numbering():
    from polara_amd.coldstart import stack_features
    frame = {'genres': [['b', 'a'], ['c'], [], ['a', 'c', 'a']], 'tags': [[1], [2, 1], [3], []]}
    F, labels = stack_features(frame)
    assert F.shape == (4, len(labels['genres']) + len(labels['tags'])) and set(labels['genres']) == {'a', 'b', 'c'}
    assert sorted(labels['tags'].values()) == [0, 1, 2] and F.nnz == 5 + 4 and (F.data == 1).all()
    dense = F.toarray()
    assert dense[3, labels['genres']['a']] == 1 and dense[3].sum() == 2 and dense[2, len(labels['genres']) + labels['tags'][3]] == 1
    F2, _ = stack_features({'genres': [['a', 'zzz'], ['zzz'], []], 'tags': [[9], [1], []]}, labels=labels)
    assert F2.shape == (3, F.shape[1]) and F2.nnz == 2          # unknown labels are dropped, the columns stay


def test_rank_truncation_and_growth():
    g = load_golden('coldstart_svd')
    m = model_for(g, ColdStartNumpyOps())
    m.build()
    full = m.factors
    m.rank = 5
    assert m.factors['itemid_features'].shape[1] == 5 and m.factors['userid'].shape[1] == 5
    assert np.allclose(np.abs(m._item_features_transform_helper), np.abs(g['G_rank5']), rtol=1e-6,
                       atol=1e-9 * np.abs(g['G_rank5']).max())
    assert ref.same_up_to_sign(m.factors['itemid_features'], g['W'][:, :5], 1e-8)
    assert full['itemid_features'].shape[1] == 10       # whoever kept the old dict keeps the full factors
    # not lower than the transform: the reference's ValueError
    m._rank = 4
    with pytest.raises(ValueError):
        m._check_reduced_rank(5)
    # the rank grows: everything is dropped and the model is not ready
    m.rank = 12
    assert not m._is_ready and m.item_features_embeddings is None and m._item_features_transform_helper is None


def test_caches_follow_the_factors_and_the_data():
    g = load_golden('coldstart_svd')
    m = model_for(g, ColdStartNumpyOps())
    m.build()
    image, order = m._user_factors_device()
    assert m._user_factors_device()[0] is image
    assert sorted(order.tolist()) == list(range(int(g['train_shape'][0])))
    norms = np.linalg.norm(image.V.numpy(), axis=1)
    assert (np.diff(norms) <= 1e-12).all()                # descending row norm
    saved = m.factors
    m.rank = 5
    assert m._user_factors_device()[0] is not image and m._user_factors_device()[0].K == 5
    m.factors = saved                                     # a rank-sweep pipeline restores the dict behind the model's back
    m._rank = 10
    m.update_item_features_transform()
    assert m._user_factors_device()[0].K == 10 and np.array_equal(m.get_recommendations(), g['recs'])
    cold = m._cold_dev
    m.data.set_test_data(holdout=(g['hold_user'], g['hold_cold'], g['hold_fdbk']))
    assert m._cold_dev is None and cold is not None and m._recommendations is None
    m.data.set_training_data((g['train_idx'][:, 0], g['train_idx'][:, 1], g['train_val']))
    assert m._user_image is None and m._features_dev is None and not m._is_ready and m.item_features_labels is None


def test_memory_guard_names_the_bytes():
    from polara_amd import coldstart
    need = coldstart.user_image_bytes(1_000_000, 50)
    assert need == 1_000_000 * 64 * 28
    assert coldstart.check_image_memory(1_000_000, 50, 2 * need) == need
    with pytest.raises(MemoryError, match=str(need)):
        coldstart.check_image_memory(1_000_000, 50, 2 * need - 2)


def test_multi_process_is_refused():
    g = load_golden('coldstart_svd')
    m = model_for(g, ColdStartNumpyOps())

    class Two:
        world, rank = 2, 0
    m.comm = Two()
    with pytest.raises(NotImplementedError):
        m.build()


@pytest.mark.parametrize('name', ['coldstart_mp', 'coldstart_mp_repr'])
def test_most_active_users(name):
    from polara_amd.coldstart import PopularityModelItemColdStart
    from polara_amd.data import ItemColdStartArrayData
    g = load_golden(name)
    idx = g['train_idx']
    shp = tuple(int(x) for x in g['train_shape'])
    n_cold = int(g['n_cold'])
    data = ItemColdStartArrayData((idx[:, 0], idx[:, 1], g['train_val']), (g['hold_user'], g['hold_cold'], g['hold_fdbk']),
                                  sps.csr_matrix(np.ones((shp[1], 1))), sps.csr_matrix(np.ones((n_cold, 1))), n_users=shp[0],
                                  n_items=shp[1], representative_users=g['repr_users'] if 'repr_users' in g else None)
    m = PopularityModelItemColdStart(data, ops=ColdStartNumpyOps())
    m.verbose = False
    m.topk = int(g['topk'])
    m.build()
    recs = m.get_recommendations()
    act = g['activity']
    assert m.method == 'MP(cs)' and recs.shape == g['recs'].shape and (recs == recs[0]).all()
    # the reference's sort is not stable: compare the activity of the listed users, ids where the counts around are distinct
    ours, theirs = act[recs[0]], act[g['recs'][0]]
    assert np.array_equal(ours, theirs) and (np.diff(ours) <= 0).all()
    pool = act if 'repr_users' not in g else act[g['repr_users']]
    for j in range(recs.shape[1]):
        if np.count_nonzero(pool == ours[j]) == 1:
            assert recs[0, j] == g['recs'][0, j]
    if 'repr_users' in g:
        assert np.isin(recs, g['repr_users']).all()
    scores = {type(x).__name__: x for x in m.evaluate('all')}
    if len(np.unique(pool[pool >= ours[-1]])) == len(pool[pool >= ours[-1]]):      # no tie at or above the cut: same users
        assert scores['Hits'].true_positive == float(g['eval_Hits_true_positive'])
