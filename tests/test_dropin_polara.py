"""Drop-in check against the REFERENCE ITSELF (build container only: skipped wherever /root/reference is absent,
never part of -m gpu): Polara's own `RecommenderData` object drives Polara's `SVDModel` / `CoffeeModel` and ours
(on the test-only NumPy double of the device ops) side by side — same data object, same events, same consumers
(`recommendations`, `evaluate`, `show_recommendations`, rank truncation, data-change notifications).  The two metric
tests at the end compare with the reference's numbers recorded in tests/golden/dropin_metrics.npz
(tests/golden/make_dropin_metrics.py) and run everywhere."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def polara():
    if not os.path.isdir(os.path.join(REF, 'polara')):
        pytest.skip('reference tree not present')
    sys.path.insert(0, os.path.join(HERE, 'golden', '_numba_shim'))   # numba is not installed: pass-through shim
    sys.path.insert(0, REF)
    import warnings
    warnings.filterwarnings('ignore')
    import polara as ref
    yield ref
    sys.path.remove(REF)


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def make_data(ref, seed=0, **cfg):
    import pandas as pd
    from polara_amd.synth import planted_csr, csr_to_coo_triplets
    u, i, v = csr_to_coo_triplets(planted_csr(400, 150, 18, 5, levels=5, seed=11, min_items=6, max_items=60))
    # external ids that are NOT the internal ones: the index translation must be exercised
    df = pd.DataFrame({'userid': 1000 + 3 * u, 'itemid': 50000 - 7 * i, 'rating': v})
    data = ref.RecommenderData(df, 'userid', 'itemid', 'rating', seed=seed)
    data.verbose = False
    for k, val in cfg.items():
        setattr(data, k, val)
    quiet(data.prepare)
    return data


def clear_rows(ref_model, topk):
    """rows of the reference whose top-(k+1) scores are pairwise distinct (the others are implementation-defined)"""
    test_data, shape, _ = ref_model._get_test_data()
    scores, sd = ref_model.slice_recommendations(test_data, shape, 0, shape[0])
    if ref_model.filter_seen:
        ref_model.downvote_seen_items(scores, sd)
    top = -np.sort(-scores, axis=1)[:, :topk + 1]
    return (np.diff(-top, axis=1) > 1e-9 * np.abs(top[:, :1])).all(axis=1)


@pytest.mark.parametrize('cfg', [dict(warm_start=True, holdout_size=3, test_ratio=0.2),
                                 dict(test_fold=4, warm_start=False, holdout_size=2, test_ratio=0.25, random_holdout=True)],
                         ids=['warm', 'known_users'])
def test_svd_model_side_by_side(polara, cfg):
    from numpy_ops import NumpyOps
    from polara_amd.models import SVDModel
    data = make_data(polara, **cfg)
    ref_m = polara.SVDModel(data)
    our_m = SVDModel(data, ops=NumpyOps())
    for m in (ref_m, our_m):
        m.verbose = False
        m.rank, m.topk = 8, 7
    np.random.seed(0)
    quiet(ref_m.build)
    our_m.build()
    assert np.allclose(our_m.factors['singular_values'], ref_m.factors['singular_values'], rtol=1e-9)
    clear = clear_rows(ref_m, 7)
    assert clear.mean() > 0.9
    assert np.array_equal(our_m.recommendations[clear], ref_m.recommendations[clear])
    # evaluate(): the reference's own metric code runs on our lists (pandas holdout) -> identical hit counts
    # wherever the lists are; give both the same lists on the tie rows to compare the numbers 1:1
    our_m._recommendations[~clear] = ref_m.recommendations[~clear]
    for a, b in zip(quiet(our_m.evaluate, 'hits'), quiet(ref_m.evaluate, 'hits')):
        assert a == b
    ra, rb = quiet(our_m.evaluate, 'relevance'), quiet(ref_m.evaluate, 'relevance')
    assert np.isclose(ra.precision, rb.precision, rtol=1e-13) and np.isclose(ra.recall, rb.recall, rtol=1e-13)
    # show_recommendations: a test user by index, and ad-hoc users by external item ids
    test_users = ref_m._get_test_data()[2]       # warm start: row numbers; known users: internal ids of the holdout users
    for row in (0, 5):
        u = row if cfg['warm_start'] else int(test_users[row])
        t_ref, s_ref = quiet(ref_m.show_recommendations, u)
        t_our, s_our = our_m.show_recommendations(u)
        assert np.array_equal(np.sort(s_ref), np.sort(s_our))
        if clear[row]:
            assert np.array_equal(t_ref, t_our)
    ext_items = data.index.itemid.training['old'].values if hasattr(data.index.itemid, 'training') else data.index.itemid['old'].values
    liked = list(ext_items[[3, 17, 42, 77]])
    before = (data.test.testset, data.test.holdout)
    t_ref, s_ref = quiet(ref_m.show_recommendations, liked, 5)
    t_our, s_our = our_m.show_recommendations(liked, topk=5)
    assert data.test.testset is before[0] and data.test.holdout is before[1]          # the data object is restored
    assert np.array_equal(np.sort(s_ref), np.sort(s_our)) and set(s_our) == set(liked)
    assert np.array_equal(t_ref, t_our) and len(t_our) == 5 and our_m.topk == 7
    # the {item: feedback} form raises inside the reference under pandas 2 (`zip` hands `.loc` a tuple,
    # models.py:300-318); ours takes it: with the list form's implied feedback (the training maximum) it must give
    # the list form's answer, and other weights a different profile but the same seen items
    with pytest.raises(Exception):
        quiet(ref_m.show_recommendations, {liked[0]: 5.0, liked[2]: 1.0}, 5)
    fmax = float(data.training['rating'].max())
    t_dict, s_dict = our_m.show_recommendations({it: fmax for it in liked}, topk=5)
    assert np.array_equal(t_dict, t_our) and set(s_dict) == set(liked)
    _, s_w = our_m.show_recommendations({liked[0]: 5.0, liked[2]: 1.0}, topk=5)
    assert set(s_w) == {liked[0], liked[2]}
    # rank truncation keeps both models ready and equal (models.py:812-832)
    ref_m.rank = our_m.rank = 4
    assert our_m._is_ready and ref_m._is_ready
    clear4 = clear_rows(ref_m, 7)
    assert np.array_equal(our_m.recommendations[clear4], ref_m.recommendations[clear4])
    # a change of the data (new split) reaches both models through the data object's events
    data.test_fold = 2 if data.test_fold != 2 else 3
    quiet(data.update)
    assert not our_m._is_ready and not ref_m._is_ready and our_m._recommendations is None


def test_coffee_model_side_by_side(polara):
    from numpy_ops import NumpyOps
    from polara_amd.models import CoffeeModel
    from polara.recommender.models import CoffeeModel as RefCoffee
    data = make_data(polara, test_fold=4, warm_start=False, holdout_size=2, test_ratio=0.25)
    ref_m, our_m = RefCoffee(data), CoffeeModel(data, ops=NumpyOps())
    for m in (ref_m, our_m):
        m.verbose = False
        m.mlrank, m.topk, m.seed = (6, 5, 3), 6, 2
        m.growth_tol = 1e-6
    quiet(ref_m.build)
    our_m.build()
    f = data.fields
    for key in (f.userid, f.itemid, f.feedback):
        a, b = our_m.factors[key], ref_m.factors[key]
        assert np.abs(a @ a.T - b @ b.T).max() < 1e-7
    assert np.isclose(np.linalg.norm(our_m.factors['core']), np.linalg.norm(ref_m.factors['core']), rtol=1e-8)
    clear = clear_rows(ref_m, 6)
    assert clear.mean() > 0.8 and np.array_equal(our_m.recommendations[clear], ref_m.recommendations[clear])
    our_m._recommendations[~clear] = ref_m.recommendations[~clear]
    for a, b in zip(quiet(our_m.evaluate, 'hits'), quiet(ref_m.evaluate, 'hits')):
        assert a == b
    # the extras of the class (models.py:1027-1092) on Polara's own data object: the holdout is a pandas frame there and
    # the level -> feedback value map is data.index.feedback
    td, shape, _ = ref_m._get_test_data()
    for mode in (0, 1, 2):
        r_unf, r_sl = ref_m.unfold_test_tensor_slice(td, shape, 2, 31, mode)
        o_unf, o_sl = our_m.unfold_test_tensor_slice(td, shape, 2, 31, mode)
        assert r_unf.shape == o_unf.shape and (r_unf != o_unf).nnz == 0 and all(np.array_equal(x, y) for x, y in zip(r_sl, o_sl))
    assert all(np.array_equal(x, y) for x, y in zip(ref_m.get_holdout_slice(2, 31), our_m.get_holdout_slice(2, 31)))
    ref_pred, our_pred = ref_m.predict_feedback(), our_m.predict_feedback()
    assert our_pred.shape == ref_pred.shape and (our_pred == ref_pred).mean() > 0.99      # (near-ties between two levels aside)
    # given OUR factors the reference's own code predicts exactly what the device kernel predicts
    ref_m.factors = dict(our_m.factors)
    assert np.array_equal(ref_m.predict_feedback(), our_pred)


def test_reference_pipelines_drive_our_model(polara):
    """The reference's own rank sweep (`evaluation/pipelines.py:81-116`: one build at the largest rank, truncation
    through the `rank` setter, `evaluate()` per rank, factors restored afterwards) run on our model and on its own."""
    from numpy_ops import NumpyOps
    from polara.evaluation.pipelines import find_optimal_svd_rank
    from polara_amd.models import SVDModel
    data = make_data(polara, warm_start=True, holdout_size=3, test_ratio=0.2)
    ref_m, our_m = polara.SVDModel(data), SVDModel(data, ops=NumpyOps())
    for m in (ref_m, our_m):
        m.verbose = False
        m.topk = 10
    ranks = [2, 4, 6, 9, 12]
    np.random.seed(0)
    # target: the hit count (the reference's `precision` is not usable as a target under numpy 2 — it comes out of
    # `np.divide(..., where=mask)` without `out=` and changes from call to call, 0.204 / 3.159 on this very model)
    kw = dict(metric_type='hits', return_scores=True)
    best_ref, scores_ref = quiet(find_optimal_svd_rank, ref_m, ranks, 'true_positive', **kw)
    best_our, scores_our = quiet(find_optimal_svd_rank, our_m, ranks, 'true_positive', **kw)
    assert len(our_m.training_time) == 1 and our_m.rank == 12 and our_m.factors[data.fields.itemid].shape[1] == 12
    # rows with tied scores may differ between the two: a hit more or less among the 240 holdout items
    assert np.abs(scores_our.values - scores_ref.values).max() <= 2, (scores_our, scores_ref)
    assert best_our == best_ref or abs(scores_ref[best_our] - scores_ref[best_ref]) <= 2
    # the pipeline put the rank-12 factors back behind the model's back: the next lists must be rank-12 lists
    clear = clear_rows(ref_m, 10)
    assert ref_m.rank == 12 and np.array_equal(our_m.recommendations[clear], ref_m.recommendations[clear])


def test_reference_tucker_rank_pipeline_drives_our_model(polara):
    """`find_optimal_tucker_ranks` (evaluation/pipelines.py:118-158): one HOOI build at the largest multilinear rank,
    every smaller one through the `mlrank` setter (core rounding, models.py:949-980), factors restored by the
    pipeline after each step."""
    from numpy_ops import NumpyOps
    from polara.evaluation.pipelines import find_optimal_tucker_ranks
    from polara.recommender.models import CoffeeModel as RefCoffee
    from polara_amd.models import CoffeeModel
    data = make_data(polara, test_fold=4, warm_start=False, holdout_size=2, test_ratio=0.25)
    ref_m, our_m = RefCoffee(data), CoffeeModel(data, ops=NumpyOps())
    for m in (ref_m, our_m):
        m.verbose = False
        m.topk, m.seed, m.growth_tol = 8, 3, 1e-6
    grid = [[3, 6], [3, 5], [2, 3]]
    kw = dict(metric_type='hits', return_scores=True)
    best_ref, scores_ref = quiet(find_optimal_tucker_ranks, ref_m, grid, 'true_positive', **kw)
    best_our, scores_our = quiet(find_optimal_tucker_ranks, our_m, grid, 'true_positive', **kw)
    assert list(scores_our.index) == list(scores_ref.index) and len(scores_our) == 8
    assert len(our_m.training_time) == 1 and our_m.mlrank == (6, 5, 3)
    assert np.abs(scores_our.values - scores_ref.values).max() <= 2, (scores_our, scores_ref)
    assert best_our == best_ref or abs(scores_ref[best_our] - scores_ref[best_ref]) <= 2
    clear = clear_rows(ref_m, 8)
    assert np.array_equal(our_m.recommendations[clear], ref_m.recommendations[clear])


def test_native_pipelines_equal_the_reference_pipelines_on_the_same_model(polara):
    """polara_amd.pipelines restates `find_optimal_tucker_ranks`, `find_optimal_config` and `random_grid`
    (evaluation/pipelines.py:23-53,119-214) without pandas: on ONE model object the reference's functions and ours must
    visit the same points, produce the same values and pick the same winner; the model is left as the reference leaves it."""
    from numpy_ops import NumpyOps
    from polara.evaluation import pipelines as ref_p
    from polara_amd import pipelines as our_p
    from polara_amd.models import CoffeeModel, SVDModel
    data = make_data(polara, test_fold=4, warm_start=False, holdout_size=2, test_ratio=0.25)
    m = CoffeeModel(data, ops=NumpyOps())
    m.verbose = False
    m.topk, m.seed, m.growth_tol = 8, 3, 1e-6
    grid = [[3, 6], [3, 5], [2, 3]]
    best_ref, scores_ref = quiet(ref_p.find_optimal_tucker_ranks, m, grid, 'true_positive', metric_type='hits', return_scores=True)
    state_ref = (m.mlrank, {k: v.copy() for k, v in m.factors.items()})
    best_our, scores_our = quiet(our_p.find_optimal_tucker_ranks, m, grid, 'true_positive', metric_type='hits', return_scores=True)
    assert list(scores_our) == list(scores_ref.index) and len(scores_our) == 8
    assert [scores_our[r] for r in scores_our] == list(scores_ref.values) and best_our == best_ref
    assert m.mlrank == state_ref[0] == (6, 5, 3) and len(m.training_time) == 1
    assert all(np.array_equal(m.factors[k], state_ref[1][k]) for k in state_ref[1])
    # same_space and the infeasible combinations are skipped alike
    b1, s1 = quiet(ref_p.find_optimal_tucker_ranks, m, [[1, 5], [1, 5], [2, 4]], 'true_positive', metric_type='hits',
                   return_scores=True, same_space=True)
    b2, s2 = quiet(our_p.find_optimal_tucker_ranks, m, [[1, 5], [1, 5], [2, 4]], 'true_positive', metric_type='hits',
                   return_scores=True, same_space=True)
    assert list(s2) == list(s1.index) == [(5, 5, 2), (5, 5, 4)] and b1 == b2
    assert [s2[r] for r in s2] == list(s1.values)

    sv = SVDModel(data, ops=NumpyOps())
    sv.verbose = False
    sv.topk = 8
    pts = [(3,), (9,), (6,)]
    cfg_ref, sc_ref = quiet(ref_p.find_optimal_config, sv, pts, ('rank',), 'true_positive', metric_type='hits', return_scores=True)
    cfg_our, sc_our = quiet(our_p.find_optimal_config, sv, pts, ('rank',), 'true_positive', metric_type='hits', return_scores=True,
                            reset_config={'rank': 4})
    assert cfg_our == cfg_ref and [sc_our[p] for p in pts] == [sc_ref[p] for p in pts]
    assert sv.rank == 4                                  # reset_config applied after the last point
    # a single (non-tuple) parameter name, as the reference allows
    cfg1 = quiet(our_p.find_optimal_config, sv, [5, 7], 'rank', 'true_positive', metric_type='hits')
    assert set(cfg1) == {'rank'} and cfg1['rank'] in (5, 7)

    params = {'rank': [2, 4, 8, 16], 'topk': [5, 10], 'seed': [0, 1, 2]}
    g, names = our_p.random_grid(params, n=10, rng=np.random.RandomState(0))
    assert names == tuple(params) and len(g) == 10 and all(len(pt) == 3 and pt[0] in params['rank'] for pt in g)
    g_all, _ = our_p.random_grid(params, n=0, rng=np.random.RandomState(1))
    assert len(g_all) == 24                              # n = 0: the whole grid, like the reference
    g_skip, _ = our_p.random_grid(params, n=0, skip_config=lambda pt: pt[0] == 16, rng=np.random.RandomState(2))
    assert len(g_skip) == 18 and all(pt[0] != 16 for pt in g_skip)
    g_ref, names_ref = ref_p.random_grid(params, n=0)
    assert g_ref == g_all and names_ref == names
    with pytest.raises(TypeError):
        our_p.random_grid(params, n=2.5)
    with pytest.raises(ValueError):
        our_p.random_grid(params, n=-1)


def test_reference_evaluation_engine_cross_validation(polara):
    """`evaluation_engine.run_cv_experiment` with `topk_test` inside (evaluation_engine.py:104-144): the data object
    moves from fold to fold (`data.update()` -> change events -> rebuild), the engine sets `topk` from large to small
    (cached lists are cut, not recomputed, models.py:123-128) — both models in ONE experiment on the shared data."""
    from numpy_ops import NumpyOps
    from polara.evaluation import evaluation_engine as ee
    from polara_amd.models import SVDModel
    data = make_data(polara, warm_start=True, holdout_size=3, test_ratio=0.2)
    ref_m, our_m = polara.SVDModel(data), SVDModel(data, ops=NumpyOps())
    our_m.method = 'PureSVD-device'
    for m in (ref_m, our_m):
        m.verbose = False
        m.rank = 7
    np.random.seed(0)
    res = quiet(ee.run_cv_experiment, [ref_m, our_m], folds=[1, 3], metrics='hits', fold_experiment=ee.topk_test,
                topk_list=[3, 10, 5])
    assert len(our_m.training_time) == 2 and len(ref_m.training_time) == 2      # one build per fold, none per topk
    ref_rows, our_rows = res.xs('PureSVD', level='model'), res.xs('PureSVD-device', level='model')
    assert list(ref_rows.index) == list(our_rows.index) and len(ref_rows) == 2 * 3          # folds x topk
    cols = [('hits', 'true_positive'), ('hits', 'false_positive'), ('hits', 'false_negative')]
    diff = np.abs(ref_rows[cols].values.astype(float) - our_rows[cols].values.astype(float))
    assert diff.max() <= 2, res                                    # rows with tied scores: a hit more or less


@pytest.mark.parametrize('variant', ['scaled', 'threshold', 'nofilter'])
def test_model_options_side_by_side(polara, variant):
    """ScaledSVD's row/column scaling, a feedback threshold on a known-user split (below-threshold test feedback is
    zeroed, not dropped: data.py:861) and `filter_seen=False`, each next to the reference on the same data object."""
    from numpy_ops import NumpyOps
    from polara.recommender.models import ScaledSVD as RefScaled
    from polara_amd.models import SVDModel, ScaledSVD
    cfg = dict(warm_start=True, holdout_size=3, test_ratio=0.2)
    if variant == 'threshold':
        cfg = dict(test_fold=4, warm_start=False, holdout_size=2, test_ratio=0.25)
    data = make_data(polara, **cfg)
    kw = dict(feedback_threshold=4) if variant == 'threshold' else {}
    ref_m = (RefScaled if variant == 'scaled' else polara.SVDModel)(data, **kw)
    our_m = (ScaledSVD if variant == 'scaled' else SVDModel)(data, ops=NumpyOps(), **kw)
    for m in (ref_m, our_m):
        m.verbose = False
        m.rank, m.topk = 6, 9
        if variant == 'scaled':
            m.col_scaling, m.row_scaling = 0.3, 0.8
        if variant == 'nofilter':
            m.filter_seen = False
    np.random.seed(0)
    quiet(ref_m.build)
    our_m.build()
    assert our_m.method == ref_m.method
    assert np.allclose(our_m.factors['singular_values'], ref_m.factors['singular_values'], rtol=1e-9)
    clear = clear_rows(ref_m, 9)      # with the threshold, users left without positive feedback score 0 everywhere
    assert clear.mean() > 0.6 and np.array_equal(our_m.recommendations[clear], ref_m.recommendations[clear])
    A_ref, A_our = ref_m.get_training_matrix(), our_m.get_training_matrix()
    assert (A_ref != A_our).nnz == 0 and A_ref.dtype == A_our.dtype
    (m_ref, td_ref), (m_our, td_our) = ref_m.get_test_matrix(), our_m.get_test_matrix()
    assert (m_ref != m_our).nnz == 0 and all(np.array_equal(a, b) for a, b in zip(td_ref, td_our))


def test_coffee_flatteners_and_rank_reduction_side_by_side(polara):
    """One HOOI build each, then every way the reference flattens the feedback mode (models.py:983-1006) and a
    reduction of the multilinear rank through the setter (core rounding, models.py:949-980)."""
    from numpy_ops import NumpyOps
    from polara.recommender.models import CoffeeModel as RefCoffee
    from polara_amd.models import CoffeeModel
    data = make_data(polara, test_fold=4, warm_start=False, holdout_size=2, test_ratio=0.25)
    ref_m, our_m = RefCoffee(data), CoffeeModel(data, ops=NumpyOps())
    for m in (ref_m, our_m):
        m.verbose = False
        m.mlrank, m.topk, m.seed, m.growth_tol = (7, 6, 4), 6, 5, 1e-6
    quiet(ref_m.build)
    our_m.build()
    for flattener in (slice(0, None), [2, 3], 3, 'sum', (slice(1, None), 'mean'), lambda t: t[..., -1] - t[..., 0]):
        ref_m.flattener = our_m.flattener = flattener
        assert our_m._recommendations is None                      # the setter flushes the cache (models.py:936-940)
        clear = clear_rows(ref_m, 6)
        assert clear.mean() > 0.7, flattener
        assert np.array_equal(our_m.recommendations[clear], ref_m.recommendations[clear]), flattener
    # flatteners that are NOT linear in the feedback factor ('max', 'min', ...) see the sign of its columns, which is
    # arbitrary in the reference (ARPACK's singular vectors): there the reference's own formula on OUR factors is the
    # yardstick (the reference model given our factors)
    for flattener in ((slice(1, None), 'max'), 'min'):
        ref_m.flattener = our_m.flattener = flattener
        saved = dict(**ref_m.factors)
        try:
            ref_m.factors = dict(**our_m.factors)
            ref_m._recommendations = None
            clear = clear_rows(ref_m, 6)
            assert clear.mean() > 0.7 and np.array_equal(our_m.recommendations[clear], ref_m.recommendations[clear]), flattener
        finally:
            ref_m.factors = saved
            ref_m._recommendations = None
    ref_m.flattener = our_m.flattener = slice(0, None)
    for mlrank in ((5, 6, 4), (5, 4, 3)):
        ref_m.mlrank = our_m.mlrank = mlrank
        assert our_m._is_ready and ref_m._is_ready
        assert our_m.factors['core'].shape == ref_m.factors['core'].shape == mlrank
        clear = clear_rows(ref_m, 6)
        assert clear.mean() > 0.7 and np.array_equal(our_m.recommendations[clear], ref_m.recommendations[clear]), mlrank
    ref_m.mlrank = our_m.mlrank = (8, 6, 4)                         # growing a rank invalidates the model
    assert not our_m._is_ready and not ref_m._is_ready


@pytest.mark.parametrize('kind', ['svd', 'coffee'])
def test_data_events_reach_both_models_alike(polara, kind):
    """A walk through the data object's configuration (data.py:166-330: some changes re-split the data — on_change,
    the model must be rebuilt — others only redraw the test part — on_update, only the lists are stale): after every
    `data.update()` our model's readiness and cache state must be the reference model's, and so must the next lists."""
    from numpy_ops import NumpyOps
    from polara.recommender.models import CoffeeModel as RefCoffee
    from polara_amd.models import SVDModel, CoffeeModel
    data = make_data(polara, warm_start=True, holdout_size=3, test_ratio=0.2)
    if kind == 'svd':
        ref_m, our_m = polara.SVDModel(data), SVDModel(data, ops=NumpyOps())
    else:
        ref_m, our_m = RefCoffee(data), CoffeeModel(data, ops=NumpyOps())
    for m in (ref_m, our_m):
        m.verbose = False
        m.topk = 8
        if kind == 'svd':
            m.rank = 6
        else:
            m.mlrank, m.seed, m.growth_tol = (5, 5, 3), 1, 1e-6

    def lists_agree():
        np.random.seed(0)
        r_ref = quiet(lambda: ref_m.recommendations)
        r_our = quiet(lambda: our_m.recommendations)
        assert r_ref.shape == r_our.shape
        clear = clear_rows(ref_m, 8)
        assert clear.mean() > 0.6 and np.array_equal(r_our[clear], r_ref[clear])

    lists_agree()
    walk = [('holdout_size', 2), ('random_holdout', True), ('test_sample', 10), ('test_sample', None), ('test_fold', 3),
            ('holdout_size', 1), ('warm_start', False), ('test_ratio', 0.25), ('test_fold', 2), ('holdout_size', 3),
            ('warm_start', True)]
    for attr, value in walk:
        setattr(data, attr, value)
        quiet(data.update)
        state_ref = (ref_m._is_ready, ref_m._recommendations is None)
        state_our = (our_m._is_ready, our_m._recommendations is None)
        assert state_our == state_ref, (attr, value, state_our, state_ref)
        lists_agree()
    assert len(our_m.training_time) == len(ref_m.training_time)            # rebuilt exactly as often


METRIC_CFGS = [dict(warm_start=True, holdout_size=3, test_ratio=0.2),
               dict(test_fold=4, warm_start=False, holdout_size=2, test_ratio=0.25, random_holdout=True),
               dict(warm_start=True, holdout_size=1, test_ratio=0.2)]
METRIC_CFG_IDS = ['warm_h3', 'known_h2', 'warm_h1']
METRIC_TOPKS = (12, 5, 1)
METRIC_SWITCH = (None, 4)


def golden_metrics():
    return np.load(os.path.join(HERE, 'golden', 'dropin_metrics.npz'))


def same_hits(got, want):
    """a Hits tuple against the recorded one (NaN where the reference returned None)"""
    assert len(got) == len(want), (got, want)
    for a, b in zip(got, want):
        assert (a is None and np.isnan(b)) or a == b, (got, want)


@pytest.mark.parametrize('cid', METRIC_CFG_IDS)
def test_native_metrics_equal_the_reference_evaluate(cid):
    """polara_amd.evaluation (what `evaluate()` runs on ArrayData / without Polara) against the reference's
    `evaluate()` on the SAME lists and holdout, over topk, switch_positive and the metric families — every number
    that does not pass through the reference's uninitialised-memory division (see evaluation.py's header).  The lists
    (the reference's SVDModel, rank 6, top-12, on Polara's own data object split as METRIC_CFGS says), the holdout and the
    reference's numbers are recorded in tests/golden/dropin_metrics.npz."""
    from polara_amd import evaluation as ev
    g = golden_metrics()
    p = cid + '/'
    recs, hu, hi_, hf = g[p + 'recs'], g[p + 'hu'], g[p + 'hi'], g[p + 'hf']
    n_items, holdout_size = int(g[p + 'n_items']), int(g[p + 'holdout_size'])
    for topk in METRIC_TOPKS:
        for switch_positive in METRIC_SWITCH:
            kw = dict(topk=topk, switch_positive=switch_positive)
            q = '%s%d_%s/' % (p, topk, switch_positive)
            got = dict((type(s).__name__, s) for s in ev.evaluate(recs, hu, hi_, hf, n_items, metric_type='all',
                                                                    holdout_size=holdout_size, **kw))
            assert sorted(got) == list(g[q + 'families'])
            same_hits(got['Hits'], g[q + 'hits'])
            assert np.isclose(got['Experience'].coverage, g[q + 'coverage'], rtol=1e-13)
            rk_got = got['Ranking']._asdict()
            for name in set(rk_got) & {'map', 'arhr', 'mrr'}:
                assert np.isclose(rk_got[name], g[q + 'ranking_' + name], rtol=1e-12), (name, topk, switch_positive)
            rl_got = got['Relevance']._asdict()
            if 'hr' in rl_got:
                assert np.isclose(rl_got['hr'], g[q + 'relevance_hr'], rtol=1e-13)


def zero_feedback_inputs():
    """seeded lists and a holdout with explicit zero ratings, two of every user's four holdout items recommended"""
    rng = np.random.RandomState(5)
    n_users, n_items, topk, per = 60, 40, 8, 4
    recs = np.stack([rng.permutation(n_items)[:topk] for _ in range(n_users)]).astype(np.int64)
    hu = np.repeat(np.arange(n_users), per)
    hi_ = np.concatenate([np.r_[recs[u, rng.permutation(topk)[:2]],                       # two recommended items ...
                                rng.permutation(np.setdiff1d(np.arange(n_items), recs[u]))[:per - 2]]
                          for u in range(n_users)])
    hf = rng.randint(0, 6, len(hu)).astype(np.float64)                                    # ... some with feedback 0
    return recs, hu, hi_, hf, n_items, topk, per


@pytest.mark.parametrize('switch_positive', [None, 3])
def test_zero_feedback_holdout_entries_count_like_the_reference(switch_positive):
    """Holdout entries with feedback exactly 0 (explicit zero ratings, ignore_feedback=False): never a hit or a miss in
    the reference (boolean image x rank matrix), dropped from the per-class counts under a positive/negative split,
    still holdout items without one (evaluation.py:60-84, 188-205).  The reference's numbers on these inputs
    (`assemble_scoring_matrices` + `get_hits` / `get_map_score` / `get_arhr_score` / `get_hr_score` / `get_mrr_score`)
    are recorded in tests/golden/dropin_metrics.npz."""
    from polara_amd import evaluation as ev
    recs, hu, hi_, hf, n_items, topk, per = zero_feedback_inputs()
    assert (hf == 0).sum() > 10 and ((hf == 0) & (np.arange(len(hf)) % per < 2)).sum() > 3
    g = golden_metrics()
    q = 'zero_%s/' % switch_positive
    got = dict((type(s).__name__, s) for s in ev.evaluate(recs, hu, hi_, hf, n_items, metric_type='all',
                                                            switch_positive=switch_positive, holdout_size=per))
    same_hits(got['Hits'], g[q + 'hits'])
    assert np.isclose(got['Ranking'].map, g[q + 'map'], rtol=1e-12)
    assert np.isclose(got['Ranking'].arhr, g[q + 'arhr'], rtol=1e-12)
    single = dict((type(s).__name__, s) for s in ev.evaluate(recs, hu, hi_, hf, n_items, metric_type=['relevance', 'ranking'],
                                                               switch_positive=switch_positive, simple_rates=True))
    assert np.isclose(single['Relevance'].hr, g[q + 'hr'], rtol=1e-13)
    assert np.isclose(single['Ranking'].mrr, g[q + 'mrr'], rtol=1e-12)
