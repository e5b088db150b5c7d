"""Item-to-item and most-popular baselines, host side (no GPU): the NumPy/SciPy restatement (tests/i2i_reference.py)
against the reference's own lists (tests/golden/i2i_*.npz, mp_*.npz from tests/golden/make_golden_i2i.py), and the
planning, memory guard and topk limits of the device path (polara_amd/i2i.py, the library's pk_i2i_* queries)."""
import numpy as np
import pytest

import i2i_reference as ref
from conftest import load_golden

I2I_FIXTURES = ['i2i_sparse', 'i2i_nofilter', 'i2i_warm', 'i2i_implicit', 'i2i_dense', 'i2i_nondyadic']
MP_FIXTURES = ['mp_count', 'mp_feedback']


@pytest.mark.parametrize('name', I2I_FIXTURES)
def test_restated_i2i_matrix_is_the_reference_one(name):
    g = load_golden(name)
    A = ref.training_matrix(g['train_idx'], g['train_val'], tuple(g['train_shape']), bool(g['implicit']))
    C = ref.i2i_matrix(A)
    n = C.shape[0]
    R = np.zeros_like(C)
    R[g['c_row'], g['c_col']] = g['c_val']
    if name == 'i2i_nondyadic':
        assert np.allclose(C, R, rtol=1e-12, atol=1e-12)
        assert not np.array_equal(C.astype(np.float32).astype(np.float64), C)    # this one needs the fp64 image
    else:
        assert np.array_equal(C, R)
        assert np.array_equal(C.astype(np.float32).astype(np.float64), C)
    assert n == int(g['train_shape'][1])


@pytest.mark.parametrize('name', I2I_FIXTURES + MP_FIXTURES)
def test_restated_lists_match_the_reference(name):
    g = load_golden(name)
    scores, cls, lists = ref.fixture_lists(g)
    assert lists.shape == g['recs'].shape
    assert ref.tie_aware_mismatches(lists, g['recs'], scores, cls) == []


def test_fixtures_cover_the_cases():
    sparse = load_golden('i2i_sparse')
    assert (sparse['recs'] < 0).any() and not bool(sparse['dense_output'])
    assert bool(sparse['sparse_downvote_changed'])          # the reference's sparse filter matters on this data
    assert (load_golden('i2i_implicit')['train_val'] < 0).any()
    assert (load_golden('i2i_dense')['train_val'] < 0).any()
    assert bool(load_golden('i2i_warm')['warm_start'])
    assert not bool(load_golden('i2i_nofilter')['filter_seen'])
    mp = load_golden('mp_count')
    s = mp['item_scores']
    assert len(np.unique(s)) < len(s)                          # tied counts
    assert np.array_equal(s, ref.popularity_scores(mp['train_idx'], mp['train_val'], int(mp['test_shape'][1])))
    fb = load_golden('mp_feedback')
    assert np.array_equal(fb['item_scores'], ref.popularity_scores(fb['train_idx'], fb['train_val'],
                                                                   int(fb['test_shape'][1]), True))


def test_select_orders_by_class_score_item():
    scores = np.array([[3.0, 0.0, 3.0, -1.0, 5.0, 0.0]])
    seen = np.array([[False, False, False, False, True, False]])
    assert ref.select(scores, seen, 6, True, True).tolist() == [[0, 2, 3, -1, -1, -1]]
    assert ref.select(scores, seen, 6, True, False).tolist() == [[0, 2, 1, 5, 3, 4]]
    assert ref.select(scores, seen, 3, False, True).tolist() == [[4, 0, 2]]
    assert ref.select(scores, seen, 6, False, False).tolist() == [[4, 0, 2, 1, 5, 3]]


def test_planning_matches_the_library():
    from polara_amd import _lib, i2i
    lib = _lib.load()
    assert lib.pk_i2i_max_topk() == i2i.MAX_TOPK >= 1024
    assert lib.pk_i2i_window() == i2i.WINDOW and lib.pk_i2i_build_window() == i2i.BUILD_WINDOW
    for n_items in (1, 7, 8, 9, 2047, 2048, 2049, 26744, 100000):
        assert lib.pk_i2i_ld(n_items) == i2i.leading_dim(n_items)
        assert i2i.leading_dim(n_items) % 8 == 0 and i2i.leading_dim(n_items) >= n_items
    for n_users, n_items, topk in ((1, 5, 1), (138493, 26744, 10), (138493, 26744, 1024), (10, 3000, 100),
                                   (5, 1, 1), (0, 10, 1), (10, 10, 0), (10, 5000, 1025)):
        assert lib.pk_i2i_chunk_users(n_users, n_items, topk) == i2i.chunk_users(n_users, n_items, topk)
        assert lib.pk_i2i_topk_work_bytes(n_users, n_items, topk) == i2i.topk_work_bytes(n_users, n_items, topk)


def test_window_planning():
    from polara_amd import i2i
    assert i2i.n_windows(2048) == 1 and i2i.n_windows(2049) == 2 and i2i.n_windows(26744) == 14
    # ML-20M shape: the candidate lists of every user fit one launch pair at topk 10; at topk 1024 users are chunked
    assert i2i.chunk_users(138493, 26744, 10) == 138493
    c = i2i.chunk_users(138493, 26744, 1024)
    assert 1 <= c < 138493 and c * 14 * 1024 * 12 <= i2i.CAND_BUDGET
    assert i2i.pow2(1) == 1 and i2i.pow2(10) == 16 and i2i.pow2(1024) == 1024


def test_memory_guard():
    from polara_amd import i2i
    assert i2i.build_image_bytes(26744) == 26744 * 26744 * 8
    assert i2i.check_build_memory(26744, 2 * 26744 * 26744 * 8) == 26744 * 26744 * 8
    with pytest.raises(MemoryError, match='GB'):
        i2i.check_build_memory(26744, 2 * 26744 * 26744 * 8 - 16)
    with pytest.raises(MemoryError, match=r'5\.72 GB'):
        i2i.check_build_memory(26744, 1e9)


def test_topk_limits():
    from polara_amd import i2i
    assert i2i.check_topk(1024, 5000) == 1024
    with pytest.raises(ValueError, match='1024'):
        i2i.check_topk(1025, 5000)
    with pytest.raises(ValueError, match='out of bounds'):
        i2i.check_topk(11, 10)
    assert i2i.check_topk(2000, 2000, limit=None) == 2000


def test_models_are_exported():
    import polara_amd
    from polara_amd.models import CooccurrenceModel, PopularityModel, RecommenderModel
    assert polara_amd.CooccurrenceModel is CooccurrenceModel and polara_amd.PopularityModel is PopularityModel
    assert issubclass(CooccurrenceModel, RecommenderModel) and issubclass(PopularityModel, RecommenderModel)
    assert {'CooccurrenceModel', 'PopularityModel'} <= set(polara_amd.__all__)


def test_model_attributes_without_a_device():
    from polara_amd.data import ArrayData
    from polara_amd.models import CooccurrenceModel, PopularityModel
    u, i, v = np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([1.0, 2.0, 3.0])
    data = ArrayData((u, i, v), n_users=2, n_items=2)
    m = CooccurrenceModel(data)
    assert (m.method, m.implicit, m.dense_output, m._item_rank) == ('item-to-item', False, False, None)
    p = PopularityModel(data)
    assert (p.method, p.by_feedback_value) == ('MP', False)


def test_multi_process_raises():
    from polara_amd.data import ArrayData
    from polara_amd.models import CooccurrenceModel, PopularityModel

    class TwoRanks:
        world, rank = 2, 0
    data = ArrayData((np.array([0, 1]), np.array([0, 1]), np.ones(2)), n_users=2, n_items=2)
    for cls in (CooccurrenceModel, PopularityModel):
        with pytest.raises(NotImplementedError):
            cls(data, comm=TwoRanks()).build()
