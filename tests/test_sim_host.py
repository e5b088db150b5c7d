"""SimilarityAggregation / SIM(cs) without a device: the restatement of tests/sim_reference.py against the reference's own
lists (tests/golden/sim_*.npz, simcs_*.npz), the cases the fixtures are there for, the cold-similarity property of the data
layer, the planning queries against their Python mirrors, and the argument errors the models raise before any device call."""
import numpy as np
import pytest
import scipy.sparse as sps

import i2i_reference as ref
import sim_reference as sim
from conftest import load_golden

SIM_FIXTURES = ['sim_sparse', 'sim_nofilter', 'sim_warm', 'sim_implicit', 'sim_dense', 'sim_nonsym']
SIMCS_FIXTURES = ['simcs_sparse', 'simcs_full', 'simcs_implicit']


@pytest.fixture(scope='module')
def restated():
    """name -> (fixture, scores, classes, lists): computed once, shared, never written."""
    out = {}
    for name in SIM_FIXTURES + SIMCS_FIXTURES:
        g = load_golden(name)
        out[name] = (g,) + sim.fixture_lists(g)
    return out


@pytest.mark.parametrize('name', SIM_FIXTURES + SIMCS_FIXTURES)
def test_restatement_reproduces_the_reference(name, restated):
    g, scores, cls, lists = restated[name]
    assert lists.shape == g['recs'].shape
    assert ref.tie_aware_mismatches(lists, g['recs'], scores, cls, tol=0.0) == []
    rows = g['score_rows']
    assert np.array_equal(scores[rows], g['scores'])            # SciPy's product here = the reference's, bit for bit


def test_fixtures_cover_their_cases(restated):
    g = restated['sim_sparse'][0]
    assert (g['recs'] < 0).any() and bool(g['sparse_downvote_changed']) and not bool(g['dense_output'])
    assert not np.array_equal(g['recs'], g['recs_unmodified'])
    assert not bool(restated['sim_nofilter'][0]['filter_seen']) and bool(restated['sim_warm'][0]['warm_start'])
    g = restated['sim_implicit'][0]
    assert bool(g['implicit']) and (g['test_fdbk'] == 0).any() and (g['test_fdbk'] < 0).any()
    g = restated['sim_dense'][0]
    assert bool(g['dense_output']) and int(g['topk']) == 20 and not (g['recs'] < 0).any()
    for name in SIM_FIXTURES:
        assert restated[name][0]['test_shape'][0] >= 50, name
    g = restated['sim_nonsym'][0]
    S = sim.similarity(g)
    assert (S != S.T).nnz > 0
    assert not np.array_equal(g['recs'], g['recs_other'])
    o_scores, o_cls, o_lists = sim.sim_lists(g, dense_output=not bool(g['dense_output']))
    assert ref.tie_aware_mismatches(o_lists, g['recs_other'], o_scores, o_cls, tol=0.0) == []
    assert (restated['simcs_sparse'][0]['recs'] < 0).any() and not (restated['simcs_full'][0]['recs'] < 0).any()
    assert bool(restated['simcs_implicit'][0]['implicit'])
    assert not sim.cold_similarity(restated['simcs_sparse'][0]).has_sorted_indices      # the stored order matters


def _cold_data(cold_relations=None, n_items=6, n_cold=5):
    from polara_amd import ItemColdStartSimilarityArrayData
    train = (np.array([0, 0, 1, 2, 3]), np.array([0, 1, 2, 3, 5]), np.ones(5))
    holdout = (np.array([0, 1, 2, 3, 1]), np.array([0, 1, 2, 3, 4]), np.ones(5))
    item_features = sps.csr_matrix(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0],
                                             [0, 1, 0, 0]], dtype=np.float64))      # label 3: no training item has it
    cold_features = [[0], [3], [1, 2], [], [2]]               # cold items 1 and 3 share no label with a training item
    kw = {} if cold_relations is None else {'cold_relations_matrices': {'itemid': cold_relations}}
    return ItemColdStartSimilarityArrayData(train, holdout, item_features, cold_features, n_users=4, n_items=n_items,
                                            relations_matrices={'itemid': None, 'userid': None},
                                            relations_indices={'itemid': None, 'userid': None}, **kw)


def test_cold_items_similarity():
    assert _cold_data().cold_items_similarity is None
    rng = np.random.default_rng(3)
    M = np.round(rng.random((5, 6)), 2) * (rng.random((5, 6)) < 0.6)
    for given in (M, sps.csr_matrix(M), sps.coo_matrix(M)):
        data = _cold_data(given)
        assert list(data.cold_items_kept) == [0, 2, 4]
        C = data.cold_items_similarity
        assert sps.issparse(C) and C.format == 'csr' and C.dtype == np.float64 and C.shape == (3, 6)
        assert np.array_equal(C.toarray(), M[[0, 2, 4]])
        assert data.cold_items_similarity is C                 # kept until the cold items change
    # the stored order of a row is kept (the sums follow it)
    rows = sps.csr_matrix((np.array([.3, .1, .2]), np.array([4, 0, 2]), np.array([0, 3, 3, 3, 3, 3])), shape=(5, 6))
    assert list(_cold_data(rows).cold_items_similarity.indices) == [4, 0, 2]
    # a new holdout with other features: other cold items survive, the property follows
    data = _cold_data(M)
    data.set_test_data(holdout=(np.array([0, 1]), np.array([1, 3]), np.ones(2)),
                       cold_item_features=[[3], [0], [3], [1], []])
    assert list(data.cold_items_kept) == [1, 3] and np.array_equal(data.cold_items_similarity.toarray(), M[[1, 3]])
    with pytest.raises(ValueError, match='cold item relations'):
        _cold_data(M[:, :5]).cold_items_similarity


def test_planning_queries_equal_their_mirrors():
    from polara_amd import _lib, i2i, simagg
    lib = _lib.load()
    assert simagg.WINDOW == lib.pk_i2i_window() == 4 * simagg.QUARTER and simagg.MAX_TOPK == lib.pk_i2i_max_topk()
    assert simagg.LDS_BYTES == 2048 * 12 + 256
    for n_rows, n_cols, topk in [(1, 1, 1), (100, 300, 10), (104, 2048, 50), (13, 2049, 1024), (138493, 26744, 10),
                                 (5349, 138493, 10), (400000, 138493, 1024), (7, 6200, 100)]:
        assert lib.pk_spsp_topk_work_bytes(n_rows, n_cols, topk) == simagg.topk_work_bytes(n_rows, n_cols, topk)
        assert simagg.chunk_rows(n_rows, n_cols, topk) == lib.pk_i2i_chunk_users(n_rows, n_cols, topk)
        assert simagg.n_windows(n_cols) == i2i.n_windows(n_cols) == -(-n_cols // 2048)
    assert simagg.chunk_rows(400000, 138493, 1024) < 400000     # rows are chunked under the candidate budget
    assert simagg.check_shapes((3, 5), (5, 9)) == (3, 5, 9)
    with pytest.raises(ValueError, match='columns'):
        simagg.check_shapes((3, 5), (4, 9))


class _NoDevice:
    """stands where the device backend would: any use fails the test"""

    def __getattr__(self, name):
        raise AssertionError('the device backend was touched (%s)' % name)


def test_argument_errors_come_before_any_device_call():
    from polara_amd import ArrayData, SimilarityAggregation, SimilarityAggregationItemColdStart, SimilarityArrayData
    train = (np.array([0, 0, 1, 2, 3]), np.array([0, 1, 2, 3, 5]), np.ones(5))
    hold = (np.arange(4), np.array([2, 3, 4, 0]), np.ones(4))
    for data in (ArrayData(train, n_users=4, n_items=6, holdout=hold),
                 SimilarityArrayData(train, n_users=4, n_items=6, holdout=hold,
                                     relations_matrices={'itemid': None}, relations_indices={'itemid': None})):
        m = SimilarityAggregation(data, ops=_NoDevice())
        assert m.method == 'SIM' and m.implicit is False and m.dense_output is False
        with pytest.raises(ValueError, match='item relations'):
            m.build()
    m = SimilarityAggregationItemColdStart(_cold_data(np.ones((5, 6))), ops=_NoDevice())
    assert m.method == 'SIM(cs)' and m.filter_seen is False
    m.dense_output = True
    for call in (m.build, m.get_recommendations, m.slice_recommendations):
        with pytest.raises(NotImplementedError, match='reference'):
            call()
    m = SimilarityAggregationItemColdStart(_cold_data(), ops=_NoDevice())
    with pytest.raises(ValueError, match='cold_items_similarity'):
        m.get_recommendations()
