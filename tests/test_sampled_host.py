"""Sampled-negatives evaluation, host side (no GPU): the data mixin, the argument checks, `evaluate` on column positions
against the metric values the reference computed for the fixtures (tests/golden/make_golden_sampled.py), and the properties
of the sampler as tests/sampled_reference.py restates it."""
import numpy as np
import pytest

import sampled_reference as ref
from conftest import load_golden

FIXTURES = ('sampled_h1', 'sampled_h3', 'sampled_known')


def fixture_data(g, with_unseen=True, **kw):
    from polara_amd.data import RandomSampleArrayData
    shp = tuple(int(x) for x in g['train_shape'])
    idx = g['train_idx']
    d = RandomSampleArrayData((idx[:, 0], idx[:, 1], g['train_val']), n_users=shp[0], n_items=shp[1],
                              test=(g['test_user'], g['test_item'], g['test_fdbk']),
                              holdout=(g['hold_user'], g['hold_item'], g['hold_fdbk']), warm_start=bool(g['warm_start']), **kw)
    if with_unseen:
        d.set_unseen_interactions(g['unseen'])
    return d


def test_exports():
    import polara_amd
    names = {'RandomSampleEvaluationMixin', 'RandomSampleArrayData', 'RandomSampleEvaluationSVDMixin', 'SVDModelSampled',
             'ScaledSVDSampled'}
    assert names <= set(polara_amd.__all__)
    from polara_amd import SVDModelSampled, RandomSampleEvaluationSVDMixin, SVDModel
    assert issubclass(SVDModelSampled, RandomSampleEvaluationSVDMixin) and issubclass(SVDModelSampled, SVDModel)


@pytest.mark.parametrize('name', FIXTURES)
def test_data_mixin_positions_and_shapes(name):
    g = load_golden(name)
    d = fixture_data(g, with_unseen=False, seed=5)
    assert d.unseen_interactions is None and d.unseen_items_num is None and d._holdout_item_prefix == 'x' and d.seed == 5
    h = int(g['holdout_size'])
    assert d.holdout_size == h
    d.set_unseen_interactions(g['unseen'].astype(np.int32))
    assert d.unseen_items_num == g['unseen'].shape[1] and d.unseen_interactions.dtype == np.int64
    assert np.array_equal(d.unseen_interactions, g['unseen'])
    assert np.array_equal(d.adapt_holdout(), np.tile(np.arange(h), len(g['hold_user']) // h))      # the reference's cumcount
    assert np.array_equal(d.holdout_positions, d.adapt_holdout())
    n = g['unseen'].shape[0]
    with pytest.raises(ValueError):
        d.set_unseen_interactions([[1, 2, 3]] * (n - 1) + [[1, 2]])                 # ragged
    with pytest.raises(ValueError):
        d.set_unseen_interactions(g['unseen'][:-1])                                 # a row short
    with pytest.raises(ValueError):
        d.set_unseen_interactions(g['unseen'].ravel())                              # not a matrix
    with pytest.raises(ValueError):
        d.set_unseen_interactions(g['unseen'].astype(np.float64))
    bad = g['unseen'].copy()
    bad[0, 0] = d.n_items
    with pytest.raises(ValueError):
        d.set_unseen_interactions(bad)
    with pytest.raises(NotImplementedError):
        d.set_unseen_interactions(g['unseen'], reindex=True)
    assert np.array_equal(d.unseen_interactions, g['unseen'])                       # failed calls left the stored lists alone
    # new test data: the stored lists belonged to the former test users
    d.set_test_data(testset=(g['test_user'], g['test_item'], g['test_fdbk']), holdout=(g['hold_user'], g['hold_item'], g['hold_fdbk']))
    assert d.unseen_interactions is None and d.holdout_positions is None and d.unseen_items_num == g['unseen'].shape[1]


def test_positions_of_an_uneven_holdout():
    from polara_amd.data import RandomSampleArrayData
    d = RandomSampleArrayData(([0, 1, 2, 3], [0, 1, 2, 3], [1.0] * 4), n_users=4, n_items=9,
                              holdout=([3, 0, 3, 3, 2], [4, 5, 6, 7, 8], [1.0] * 5))
    assert np.array_equal(d.test.holdout.userid, [0, 2, 3, 3, 3])
    assert np.array_equal(d.adapt_holdout(), [0, 0, 0, 1, 2])


class _NoOps:
    """a model under test here never reaches the device"""

    def __getattr__(self, name):
        raise AssertionError('the device was asked for ' + name)


def fixture_model(g, **kw):
    from polara_amd import SVDModelSampled
    d = fixture_data(g, **kw)
    m = SVDModelSampled(d, ops=_NoOps())
    m.verbose = False
    m.topk = int(g['topk'])
    return m


def test_prediction_target_and_parent_path():
    g = load_golden('sampled_h1')
    m = fixture_model(g)
    assert m._prediction_target == 'x_itemid' and m._prediction_key == 'userid'
    m._prediction_target = m.data.fields.itemid
    m._is_ready = True
    with pytest.raises(AssertionError, match='the device was asked'):             # the parent's full-catalogue pass
        m.get_recommendations()


def test_value_errors():
    g = load_golden('sampled_h1')
    m = fixture_model(g)
    m._recommendations, m._is_ready = g['recs'], True
    for kind in ('all', 'experience', ['relevance', 'experience']):
        with pytest.raises(ValueError):
            m.evaluate(kind)
    # holdout_size must be fixed and >= 1
    m.data.holdout_size = 0
    with pytest.raises(ValueError):
        m._holdout_items()
    m.data.holdout_size = 2                                                         # 100 entries in pairs: users differ inside a pair
    with pytest.raises(ValueError):
        m._holdout_items()
    m.data.holdout_size = 1
    assert np.array_equal(m._holdout_items(), g['hold_item'][:, None])

    class Two:
        world, rank = 2, 0
    m.comm = Two()
    m._recommendations = None
    with pytest.raises(NotImplementedError):
        m.get_recommendations()


def test_checks_of_the_operators():
    from polara_amd import sampled
    assert sampled.check_candidate_shapes((7, 5), (30, 5), (7, 11), 3) == (7, 5, 30, 11)
    with pytest.raises(ValueError):
        sampled.check_candidate_shapes((7, 5), (30, 4), (7, 11), 3)
    with pytest.raises(ValueError):
        sampled.check_candidate_shapes((7, 5), (30, 5), (6, 11), 3)
    with pytest.raises(ValueError):
        sampled.check_candidate_shapes((7, 5), (30, 5), (77,), 3)
    sampled.check_sample_request(8, 64, 10, 10, 8192)
    for bad in ((0, 64, 10, 10), (65, 64, 10, 10), (8, 64, 9, 10), (9000, 10000, 10, 10)):
        with pytest.raises(ValueError):
            sampled.check_sample_request(*bad, 8192)
    # the union of the two rows counts: user 0 has 2 + 1 distinct items excluded, user 1 has item 3 in both rows, user 2 none
    t_ptr, t_idx = np.array([0, 2, 4, 4]), np.array([0, 5, 3, 4])
    h_ptr, h_idx = np.array([0, 1, 2, 2]), np.array([2, 3])
    assert sampled.users_short_of_items(t_ptr, t_idx, h_ptr, h_idx, 6, 3).tolist() == []
    assert sampled.users_short_of_items(t_ptr, t_idx, h_ptr, h_idx, 6, 4).tolist() == [0]
    assert sampled.users_short_of_items(t_ptr, t_idx, h_ptr, h_idx, 6, 5).tolist() == [0, 1]
    assert sampled.users_short_of_items(t_ptr, t_idx, None, None, 6, 5).tolist() == [0, 1]
    assert sampled.fewest_eligible_items(t_ptr, t_idx, h_ptr, h_idx, 6) == 3 and sampled.fewest_eligible_items(t_ptr, t_idx, None, None, 6) == 4
    seeds = sampled.user_seeds(42, 5)
    assert seeds.dtype == np.uint32 and np.array_equal(seeds, np.random.SeedSequence(42).generate_state(5))


@pytest.mark.parametrize('name', FIXTURES)
def test_evaluate_on_positions_gives_the_reference_metrics(name):
    g = load_golden(name)
    m = fixture_model(g)
    m._recommendations, m._is_ready = g['recs'], True
    for kind in ('relevance', 'ranking', 'hits'):
        got = m.evaluate(kind)
        names, want = [str(x) for x in g['metric_%s_names' % kind]], g['metric_%s' % kind]
        assert list(got._fields) == names, kind
        for field, w in zip(names, want):
            v = getattr(got, field)
            if np.isnan(w):                 # a field the reference leaves at None
                assert v is None or np.isnan(v), (kind, field)
            else:
                assert v == pytest.approx(w, rel=1e-12, abs=0), (kind, field)
    both = m.evaluate(['relevance', 'ranking'])
    assert len(both) == 2 and both[0] == m.evaluate('relevance')
    cut = m.evaluate('relevance', topk=5)
    assert cut == type(cut)(*m.evaluate('relevance', topk=5)) and m.topk == int(g['topk'])


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_reproduces_the_fixture(name):
    g = load_golden(name)
    h = int(g['holdout_size'])
    cand = np.concatenate((g['hold_item'].reshape(-1, h), g['unseen']), axis=1)
    lists, scores = ref.candidates_topk(g['user_factors'], g['V'], cand, int(g['topk']))
    assert np.array_equal(scores, g['scores']) and np.array_equal(lists, g['recs'])
    assert (g['min_gap'] > 1e-6 * np.abs(g['scores']).max()).all()


def test_selection_order():
    s = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, np.nan, 2.0]])
    assert ref.select(s, 7).tolist() == [[1, 2, 6, 0, 3, 4, 5]]


# ---- the sampler's definition ----------------------------------------------------------------------------------------------
def test_sampler_properties():
    rng = np.random.RandomState(0)
    n_items, n = 97, 12
    rows = [np.sort(rng.choice(n_items, k, replace=False)) for k in (0, 5, 40, 85)]
    t_ptr = np.r_[0, np.cumsum([len(r) for r in rows])]
    t_idx = np.concatenate(rows).astype(np.int32)
    h_ptr, h_idx = np.array([0, 1, 1, 3, 3]), np.array([0, 96, 1], dtype=np.int32)
    seeds = np.random.SeedSequence(7).generate_state(4)
    out = ref.sample_unseen(t_ptr, t_idx, h_ptr, h_idx, n_items, n, seeds)
    assert out.shape == (4, n) and out.dtype == np.int32
    for u in range(4):
        ex = set(rows[u].tolist()) | set(h_idx[h_ptr[u]:h_ptr[u + 1]].tolist())
        assert not ex & set(out[u].tolist())                     # nothing excluded is drawn
        assert len(set(out[u].tolist())) == n                    # no duplicates
        assert out[u].min() >= 0 and out[u].max() < n_items
    assert np.array_equal(out, ref.sample_unseen(t_ptr, t_idx, h_ptr, h_idx, n_items, n, seeds))
    other = ref.sample_unseen(t_ptr, t_idx, h_ptr, h_idx, n_items, n, np.random.SeedSequence(8).generate_state(4))
    assert all(not np.array_equal(out[u], other[u]) for u in range(4))
    # user 3 has 97 - 85 = 12 eligible items: all of them come out
    assert sorted(out[3].tolist()) == sorted(set(range(n_items)) - set(rows[3].tolist()))
    with pytest.raises(ValueError):
        ref.sample_unseen_row(1, n_items, rows[3], 13)
    # a longer sample starts with the shorter one
    assert ref.sample_unseen_row(seeds[1], n_items, rows[1], 20)[:n] == out[1].tolist()


def test_sampler_rejection_keeps_the_mapping_unbiased():
    # n_items = 3 * 2^30: 2^32 mod n_items = 2^30, a quarter of the draws are rejected, the rest map 1:1 onto the items
    n_items = 3 << 30
    got = [ref.draw(11, t, n_items) for t in range(4000)]
    rejected = sum(x is None for x in got)
    assert 850 < rejected < 1150                                  # 1000 +- 5.5 sigma (sigma = sqrt(4000 * 3/16) = 27.4)
    assert all(0 <= x < n_items for x in got if x is not None)
    assert all(ref.draw(11, t, 64) is not None for t in range(200))      # a power of two rejects nothing


def test_sampler_uniformity():
    """n_items = 64, 16 excluded, n = 8, 6000 users with one profile and distinct seeds: every eligible item is drawn
    6000 * 8 / 48 = 1000 times on average with standard deviation sqrt(1000 * (1 - 1/48)) = 31.3; 174 is 5.6 of them."""
    excluded = list(range(0, 64, 4))
    seeds = np.random.SeedSequence(2024).generate_state(6000)
    counts = np.zeros(64, dtype=np.int64)
    for s in seeds:
        counts[ref.sample_unseen_row(s, 64, excluded, 8)] += 1
    assert counts[excluded].sum() == 0 and counts.sum() == 48000
    eligible = np.delete(counts, excluded)
    assert len(eligible) == 48 and np.abs(eligible - 1000).max() <= 174, eligible
