"""Probabilistic matrix factorisation, host side (no GPU): the blocked schedule (polara_amd/pmf.py: block_schedule), the NumPy
restatement of the device's sweep (tests/pmf_reference.py) against the reference's own fixtures (tests/golden/pmf_*.npz from
tests/golden/make_golden_pmf.py), and the model's orchestration on a CPU double of the device operators.

Tolerance: every comparison with the reference is at 4 x the fixture's `restatement_gap` — the distance the generator measured
between the restatement and the reference (they differ in the summation order of `pm @ qn` alone)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import pmf_reference as ref
from conftest import load_golden
from polara_amd import pmf
from test_coldstart_host import EVAL_KEYS

FIXTURES = ['pmf_std', 'pmf_b4', 'pmf_b32', 'pmf_rank7', 'pmf_rank40', 'pmf_adagrad', 'pmf_rmsprop', 'pmf_early']


def within(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.abs(a - b).max() <= tol


@functools.lru_cache(maxsize=None)
def restated_solution(name):
    """(P, Q, RMSE history) of the restatement on a fixture: computed once, shared with the device tests, never written to"""
    g = load_golden(name)
    out = ref.solve(ref.fixture_plan(g), g['P0'], g['Q0'], **ref.solver_args(g))
    for a in out:
        a.setflags(write=False)
    return out


def seen_of(g):
    users = g['test_users']
    idx, shp = g['train_idx'], tuple(int(x) for x in g['train_shape'])
    train = sps.csr_matrix((g['train_val'], (idx[:, 0], idx[:, 1])), shape=shp)[users].tocoo()
    return train.row, train.col


def interactions(seed=0, n_users=40, n_items=30, density=0.2):
    rng = np.random.RandomState(seed)
    mask = rng.rand(n_users, n_items) < density
    mask[rng.randint(n_users, size=3)] = False          # users without interactions
    mask[:, rng.randint(n_items, size=3)] = False       # items without interactions
    u, i = np.nonzero(mask)
    return u.astype(np.int64), i.astype(np.int64), rng.randint(1, 6, size=len(u)).astype(np.float64), n_users, n_items


# ---- the schedule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', [1, 2, 3, 7, 16, 30])
def test_schedule_is_a_conflict_free_permutation(blocks):
    u, i, _, n_users, n_items = interactions(blocks)
    perm, block_ptr = pmf.block_schedule(u, i, n_users, n_items, blocks)
    B = blocks
    assert np.array_equal(np.sort(perm), np.arange(len(u)))
    assert block_ptr.shape == (B * B + 1,) and block_ptr[0] == 0 and block_ptr[-1] == len(u) and (np.diff(block_ptr) >= 0).all()
    su, si = u[perm], i[perm]
    for s in range(B):
        ranges = []
        for b in range(B):
            lo, hi = block_ptr[s * B + b], block_ptr[s * B + b + 1]
            assert (np.diff(perm[lo:hi]) > 0).all()                      # the canonical order is kept inside a block
            if hi > lo:
                ranges.append((su[lo:hi].min(), su[lo:hi].max(), si[lo:hi].min(), si[lo:hi].max()))
        for a in range(len(ranges)):                                     # user ranges and item ranges pairwise disjoint
            for c in range(a + 1, len(ranges)):
                x, y = ranges[a], ranges[c]
                assert x[1] < y[0] or y[1] < x[0]
                assert x[3] < y[2] or y[3] < x[2]
    if B == 1:
        assert np.array_equal(perm, np.arange(len(u)))


def test_parts_are_balanced_by_interaction_count():
    u, i, _, n_users, n_items = interactions(3, 200, 120, 0.3)
    B = 8
    perm, block_ptr = pmf.block_schedule(u, i, n_users, n_items, B)
    per_user_part = np.zeros(B, dtype=np.int64)
    for s in range(B):
        for b in range(B):
            per_user_part[b] += block_ptr[s * B + b + 1] - block_ptr[s * B + b]
    heaviest_user = np.bincount(u).max()
    assert per_user_part.max() - per_user_part.min() <= 2 * heaviest_user


def test_schedule_rejects_bad_block_counts():
    u, i, _, n_users, n_items = interactions(1)
    for bad in (0, -1, n_items + 1, n_users + 1):
        with pytest.raises(ValueError, match='blocks'):
            pmf.block_schedule(u, i, n_users, n_items, bad)
    perm, block_ptr = pmf.block_schedule(u, i, n_users, n_items, n_items)          # as many blocks as items: legal, mostly empty
    assert np.array_equal(np.sort(perm), np.arange(len(u))) and (np.diff(block_ptr) == 0).any()


def test_empty_input_and_single_entries():
    e = np.zeros(0, dtype=np.int64)
    perm, block_ptr = pmf.block_schedule(e, e, 5, 4, 3)
    assert len(perm) == 0 and not block_ptr.any()
    perm, block_ptr = pmf.block_schedule(np.array([2]), np.array([1]), 5, 4, 4)
    assert perm.tolist() == [0] and block_ptr[-1] == 1


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_plans_are_reproduced(name):
    g = load_golden(name)
    idx, shp = g['train_idx'], g['train_shape']
    perm, block_ptr = pmf.block_schedule(idx[:, 0], idx[:, 1], int(shp[0]), int(shp[1]), int(g['blocks']))
    assert np.array_equal(perm, g['perm']) and np.array_equal(block_ptr, g['block_ptr'])
    stats = pmf.schedule_stats(block_ptr, int(g['blocks']))
    assert stats['empty_blocks'] == int(g['empty_blocks']) and stats['longest_block'] == int(g['longest_block'])
    assert stats['launches_per_epoch'] == int(g['blocks']) + 1 and stats['strata'] == int(g['blocks'])


def test_canonical_interactions():
    u, i, v = np.array([3, 0, 3, 1, 0]), np.array([1, 2, 1, 0, 0]), np.array([1., 2., 3., 4., 5.])
    cu, ci, cv = pmf.canonical_interactions(u, i, v, (4, 3))
    assert cu.tolist() == [0, 0, 1, 3] and ci.tolist() == [0, 2, 0, 1] and cv.tolist() == [5., 2., 4., 4.]
    with pytest.raises(ValueError, match='feedback 0'):
        pmf.canonical_interactions(u, i, np.array([1., 2., -1., 4., 5.]), (4, 3))
    with pytest.raises(ValueError, match='feedback 0'):
        pmf.canonical_interactions(u, i, np.array([1., 0., 3., 4., 5.]), (4, 3))


def test_the_default_block_count_follows_its_documented_rule():
    from polara_amd import machine_model as mm
    t_s, t_l, cap = (mm.value(k) for k in ('pmf_sample_s', 'pmf_launch_s', 'pmf_max_blocks'))
    assert 'profiles/' in mm.MI355X['pmf_sample_s'][1] and 'EFFECTIVE' in mm.MI355X['pmf_launch_s'][1]
    assert 1024 <= pmf.default_blocks(20_000_000, 138_493, 26_744) <= 2048          # the measured flat minimum of the epoch
    assert pmf.default_blocks(20_000_000, 138_493, 26_744) == min(int(round((2e7 * t_s / t_l) ** 0.5)), cap)
    assert pmf.default_blocks(20_000_000, 138_493, 50) == 50            # capped by min(n_users, n_items)
    assert pmf.default_blocks(10 ** 12, 10 ** 7, 10 ** 7) == cap
    assert pmf.default_blocks(0, 5, 5) == 1 and pmf.default_blocks(3, 5, 5) == 1


# ---- the restatement against the reference ------------------------------------------------------------------------------
def check_against_fixture(g, P, Q, history, scores=None, lists=None):
    tol = 4. * float(g['restatement_gap'])
    assert len(history) == len(g['rmse_history'])                       # the same stopping epoch
    assert within(P, g['P'], tol) and within(Q, g['Q'], tol) and within(history, g['rmse_history'], tol)
    if scores is None:
        full = P[g['test_users']] @ Q.T
        scores, lists = full[:g['scores'].shape[0]], ref.top_lists(full, int(g['topk']), seen=seen_of(g))
    # a score is a sum of k products of two factors each within tol: k * (|p| + |q|) * tol, and its own rounding
    k, big = P.shape[1], max(np.abs(g['P']).max(), np.abs(g['Q']).max())
    assert within(scores, g['scores'], 2 * k * big * tol + 1e-14 * k * big * big)
    assert np.array_equal(lists, g['recs'])


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_matches_the_reference(name):
    g = load_golden(name)
    check_against_fixture(g, *restated_solution(name))
    scale = max(np.abs(g['P']).max(), np.abs(g['Q']).max())
    assert float(g['restatement_gap']) <= 1e-12 * scale
    assert float(g['min_rel_gap']) >= 1e-6 and float(g['min_refined_ratio']) >= 1.01


def test_the_fixtures_cover_what_was_asked():
    g = {n: load_golden(n) for n in FIXTURES}
    cfg = lambda n: (int(g[n]['blocks']), int(g[n]['rank']), str(g[n]['adjust']), float(g[n]['learn_rate']))
    assert cfg('pmf_std') == (1, 10, 'none', 0.005) and len(g['pmf_std']['rmse_history']) == 25
    assert cfg('pmf_b4')[0] == 4 and cfg('pmf_b32')[0] == 32 and int(g['pmf_b32']['empty_blocks']) > 0
    assert cfg('pmf_rank7')[1] == 7 and cfg('pmf_rank40')[1] == 40 and ref.group_width(40) == 64
    assert cfg('pmf_adagrad') == (16, 10, 'adagrad', 0.05) and cfg('pmf_rmsprop') == (16, 10, 'rmsprop', 0.05)
    early = g['pmf_early']
    assert 5 <= len(early['rmse_history']) <= 20 < int(early['num_epochs']) and float(early['tolerance']) > 1e-4
    for x in g.values():
        assert tuple(x['train_shape']) == (300, 150) and 4000 <= len(x['train_val']) <= 6000
        key = x['train_idx'][:, 0] * 150 + x['train_idx'][:, 1]
        assert (np.diff(key) > 0).all()                                 # the canonical order is row-major


def test_one_epoch_is_the_serial_sweep_over_the_schedule():
    """the restated epoch (sample t of all blocks of a stratum at once) against the plain loop of optimize.py:129-153 over
    the permuted list, with the tree sum in place of `pm @ qn`: bit for bit, all three adjustments"""
    u, i, v, n_users, n_items = interactions(5)
    rng = np.random.RandomState(2)
    for blocks, rank, adjust in ((1, 5, None), (4, 10, 'adagrad'), (7, 17, 'rmsprop'), (16, 40, None)):
        plan = ref.make_plan(u, i, v, n_users, n_items, blocks)
        P0, Q0 = rng.normal(scale=0.1, size=(n_users, rank)), rng.normal(scale=0.1, size=(n_items, rank))
        P, Q = P0.copy(), Q0.copy()
        S = (np.zeros_like(P), np.zeros_like(Q)) if adjust else None
        got = ref.epoch(plan, P, Q, 0.05, 0.5, adjust, S)
        sP, sQ = P0.copy(), Q0.copy()
        sS = (np.zeros_like(P), np.zeros_like(Q))
        w = ref.group_width(rank)
        block_sse = np.zeros(blocks * blocks)
        for b in range(blocks * blocks):
            for t in range(plan['block_ptr'][b], plan['block_ptr'][b + 1]):
                m, n, val = plan['users'][t], plan['items'][t], plan['vals'][t]
                pm, qn = sP[m].copy(), sQ[n].copy()
                err = val - ref.tree_dot(pm[None], qn[None], w)[0]
                gp = err * qn - pm * (0.5 / plan['row_nnz'][m])
                gq = err * pm - qn * (0.5 / plan['col_nnz'][n])
                sP[m] = pm + 0.05 * ref.adjusted(adjust, gp[None], sS[0], [m], ref.GAMMA, ref.SMOOTHING)[0]
                sQ[n] = qn + 0.05 * ref.adjusted(adjust, gq[None], sS[1], [n], ref.GAMMA, ref.SMOOTHING)[0]
                block_sse[b] += err * err
        assert np.array_equal(P, sP) and np.array_equal(Q, sQ)
        if adjust:
            assert np.array_equal(S[0], sS[0]) and np.array_equal(S[1], sS[1])
        want = 0.
        for s in range(blocks):
            acc = 0.
            for b in range(blocks):
                acc += block_sse[s * blocks + b]
            want += acc
        assert got == want


# ---- the model on the CPU double ------------------------------------------------------------------------------------------
def check_pmf_model_against_fixture(m, g, build_kwargs=None):
    """method name, factor keys, factors, history, stopping epoch, scores, lists, evaluate() — shared with the device tests"""
    adjust = ref.adjust_of(g)
    m.build(**({'adjust_gradient': adjust} if build_kwargs is None else build_kwargs))
    userid, itemid = m.data.fields.userid, m.data.fields.itemid
    assert m.method == str(g['model']) == 'PMF' and set(m.factors) == {userid, itemid}
    n = g['scores'].shape[0]
    test_data, shape, users = m._get_test_data()
    assert np.array_equal(users, g['test_users'])
    s, _ = m.slice_recommendations(test_data, shape, 0, n, users)
    recs = m.get_recommendations()
    assert recs.dtype == np.int64
    check_against_fixture(g, m.factors[userid], m.factors[itemid], np.array(m.rmse_history), s, recs)
    B = int(g['blocks'])
    assert m.build_stats['blocks'] == m.build_stats['strata'] == B and m.build_stats['launches_per_epoch'] == B + 1
    assert m.build_stats['empty_blocks'] == int(g['empty_blocks']) and m.build_stats['longest_block'] == int(g['longest_block'])
    assert m.build_stats['epochs'] == len(g['rmse_history']) == len(m.iterations_time)
    scores = {type(x).__name__: x for x in m.evaluate('all')}
    for key in EVAL_KEYS:
        _, family, field = key.split('_', 2)
        assert np.isclose(getattr(scores[family], field), float(g[key]), rtol=1e-12, atol=0), key


@pytest.mark.parametrize('name', FIXTURES)
def test_model_on_the_cpu_double(name):
    g = load_golden(name)
    check_pmf_model_against_fixture(ref.model_for(g, ref.PMFNumpyOps()), g)


def test_exports_and_defaults():
    import polara_amd
    assert 'ProbabilisticMF' in polara_amd.__all__ and polara_amd.ProbabilisticMF is pmf.ProbabilisticMF
    m = polara_amd.ProbabilisticMF(ref.golden_data(load_golden('pmf_b4')), ops=ref.PMFNumpyOps())
    got = {k: getattr(m, k) for k in ('seed', 'learn_rate', 'sigma', 'num_epochs', 'rank', 'tolerance', 'rmse_history', 'show_rmse',
                                      'iterations_time', 'method', 'blocks')}
    assert got == dict(seed=None, learn_rate=0.005, sigma=1, num_epochs=25, rank=10, tolerance=1e-4, rmse_history=None,
                       show_rmse=False, iterations_time=None, method='PMF', blocks=None)
    assert m.factors == {} and m.optimizer is pmf.pmf_sgd
    assert not hasattr(polara_amd, 'KernelizedPMF')


def test_reference_style_function_objects_name_the_adjustment():
    def adagrad(grad, m, cum_sq_grad, smoothing=1e-6):
        raise AssertionError('never called: only its name is read')

    def rmsprop(*a):
        raise AssertionError

    def identity(x, *args):
        return x
    assert pmf.adjuster_name(None) is None and pmf.adjuster_name(identity) is None
    assert pmf.adjuster_name('adagrad') == pmf.adjuster_name(adagrad) == 'adagrad'
    assert pmf.adjuster_name('rmsprop') == pmf.adjuster_name(rmsprop) == 'rmsprop'
    g = load_golden('pmf_adagrad')
    check_pmf_model_against_fixture(ref.model_for(g, ref.PMFNumpyOps()), g, build_kwargs=dict(adjust_gradient=adagrad))


@pytest.mark.parametrize('asked', ['adam', 'adanorm', 'gnprop', 'gnpropz', 'something'])
def test_other_adjustments_are_refused_by_name(asked):
    g = load_golden('pmf_b4')
    m = ref.model_for(g, ref.PMFNumpyOps())

    def fn(*a):
        raise AssertionError
    fn.__name__ = asked
    for arg in (asked, fn):
        with pytest.raises(NotImplementedError, match=asked):
            m.build(adjust_gradient=arg)
    with pytest.raises(NotImplementedError, match='lambda'):
        m.build(adjust_gradient=lambda g, m: g)
    assert not m._is_ready and m.factors == {}


def test_a_replaced_optimizer_is_refused_by_name():
    g = load_golden('pmf_b4')
    m = ref.model_for(g, ref.PMFNumpyOps())

    def kernelized_pmf_sgd(*a, **kw):
        raise AssertionError
    m.optimizer = kernelized_pmf_sgd
    with pytest.raises(NotImplementedError, match='kernelized_pmf_sgd'):
        m.build()


def test_multi_process_is_refused():
    g = load_golden('pmf_b4')
    m = ref.model_for(g, ref.PMFNumpyOps())

    class Two:
        world, rank = 2, 0
    m.comm = Two()
    with pytest.raises(NotImplementedError, match='multi-process'):
        m.build()
    ops = ref.PMFNumpyOps()
    A = ops.csr_from_coo(g['train_idx'][:, 0], g['train_idx'][:, 1], g['train_val'], g['train_shape'])
    with pytest.raises(NotImplementedError, match='multi-process'):
        pmf.pmf_sgd(ops, A, 10, 0.005, 1, 2, 1e-4, comm=Two())


def test_bad_ranks_block_counts_and_feedback_raise():
    g = load_golden('pmf_b4')
    m = ref.model_for(g, ref.PMFNumpyOps())
    for rank in (0, ref.MAX_RANK + 1):
        m.rank = rank
        with pytest.raises(ValueError, match='rank'):
            m.build()
    m.rank = 10
    m.blocks = 151                                                      # more blocks than items
    with pytest.raises(ValueError, match='blocks'):
        m.build()
    ops = ref.PMFNumpyOps()
    idx = g['train_idx']
    val = g['train_val'].copy()
    val[7] = 0.
    with pytest.raises(ValueError, match='feedback 0'):
        pmf.pmf_sgd(ops, ops.csr_from_coo(idx[:, 0], idx[:, 1], val, g['train_shape']), 10, 0.005, 1, 2, 1e-4, blocks=4)
    A = ops.csr_from_coo(idx[:, 0], idx[:, 1], g['train_val'], g['train_shape'])
    with pytest.raises(ValueError, match='initial factors'):
        pmf.pmf_sgd(ops, A, 10, 0.005, 1, 2, 1e-4, blocks=4, init=(g['P0'][:-1], g['Q0']))


def test_blocks_none_uses_the_default_rule():
    g = load_golden('pmf_b4')
    m = ref.model_for(g, ref.PMFNumpyOps())
    m.blocks, m.num_epochs = None, 1
    m.build()
    assert m.build_stats['blocks'] == pmf.default_blocks(len(g['train_val']), 300, 150) >= 1


def test_a_rank_change_rebuilds_and_warm_start_raises():
    g = load_golden('pmf_b4')
    m = ref.model_for(g, ref.PMFNumpyOps())
    m.num_epochs = 2
    m.build()
    assert m._is_ready and len(m.training_time) == 1
    m.rank = 10
    assert m._is_ready                                                  # the same rank: nothing happens
    m.rank = 6
    assert not m._is_ready and m._recommendations is None
    recs = m.recommendations
    assert len(m.training_time) == 2 and m.factors['userid'].shape[1] == 6 and recs.shape == g['recs'].shape
    m.data.warm_start = True
    with pytest.raises(NotImplementedError):
        m.get_recommendations()


def test_seed_none_draws_from_the_global_generator_and_show_rmse_prints(capsys):
    np.random.seed(77)
    P, Q = pmf.initial_factors(5, 4, 3, seed=None)
    rs = np.random.RandomState(77)
    assert np.array_equal(P, rs.normal(scale=0.1, size=(5, 3))) and np.array_equal(Q, rs.normal(scale=0.1, size=(4, 3)))
    g = load_golden('pmf_b4')
    m = ref.model_for(g, ref.PMFNumpyOps())
    m.num_epochs, m.show_rmse = 2, True
    m.build()
    out = capsys.readouterr().out
    assert 'Epoch: 0. RMSE: {}'.format(m.rmse_history[0]) in out and 'Epoch: 1. RMSE: {}'.format(m.rmse_history[1]) in out
    assert m.rmse_history == list(g['rmse_history'][:2]) or within(m.rmse_history, g['rmse_history'][:2], 4 * float(g['restatement_gap']))


def test_the_library_states_its_bounds_without_a_device():
    """host-side entries: the rank bound, the work size, and the argument check that runs before anything is enqueued"""
    from polara_amd import _lib
    lib = _lib.load()
    assert lib.pk_pmf_max_rank() == ref.MAX_RANK >= 64
    assert lib.pk_pmf_work_doubles(1) == 1 and lib.pk_pmf_work_doubles(32) == 1024
    assert _lib.PK_PMF_MAX_BLOCKS == 4096
    rc = lib.pk_pmf_epoch_f64(None, 1, ref.MAX_RANK + 1, 0, None, None, None, None, None, 0, None, 0, None, None, 0.1, 0.5, 0, None, 0,
                              None, 0, 0.9, 1e-6, None, None)
    assert rc == -1 and b'rank' in lib.pk_last_error()                   # PK_E_INVALID
    rc = lib.pk_pmf_epoch_f64(None, _lib.PK_PMF_MAX_BLOCKS + 1, 10, 0, None, None, None, None, None, 0, None, 0, None, None, 0.1, 0.5,
                              0, None, 0, None, 0, 0.9, 1e-6, None, None)
    assert rc == -1 and b'blocks' in lib.pk_last_error()


# ---- the model layer these models share (models.RecommenderModel, factor_serving, coldstart) -------------------------------
def test_the_shared_serving_code_has_one_implementation():
    import polara_amd
    from polara_amd.coldstart import ItemColdStartRecommenderMixin, SVDModelItemColdStart
    from polara_amd.factor_serving import FactorQueriesMixin
    for cls in (polara_amd.LCEModel, polara_amd.ProbabilisticMF, polara_amd.ImplicitALS):
        for name in ('get_recommendations', 'slice_recommendations', '_user_rows', 'rank'):
            assert getattr(cls, name) is getattr(FactorQueriesMixin, name), (cls.__name__, name)
    cold = polara_amd.LCEModelItemColdStart
    assert cold.get_recommendations is ItemColdStartRecommenderMixin.get_recommendations
    assert cold.slice_recommendations is ItemColdStartRecommenderMixin.slice_recommendations
    assert SVDModelItemColdStart.slice_recommendations is ItemColdStartRecommenderMixin.slice_recommendations
    assert polara_amd.CooccurrenceModel.recommend_with_scores is polara_amd.SimilarityAggregation.recommend_with_scores


def _small_lce():
    import lce_reference
    m = lce_reference.model_for(load_golden('lce_std'), lce_reference.LCENumpyOps())
    m.max_iterations = 2
    return m


def _small_pmf():
    m = ref.model_for(load_golden('pmf_std'), ref.PMFNumpyOps())
    m.num_epochs = 2
    return m


def _small_ials():
    import ials_reference
    return ials_reference.model_for(ials_reference.model_case('r7'), ials_reference.IALSNumpyOps())


@pytest.mark.parametrize('make, extra', [(_small_lce, 1), (_small_pmf, 0), (_small_ials, 0)])
def test_swapped_factors_are_uploaded_again_and_a_rank_change_invalidates(make, extra):
    m = make()
    m.build()
    recs = m.get_recommendations().copy()
    userid, itemid = m.data.fields.userid, m.data.fields.itemid
    kept = m._factors_dev
    m.factors = {k: v.copy() for k, v in m.factors.items()}
    assert np.array_equal(m.get_recommendations(), recs)
    assert m._factors_dev is not kept and m._factors_dev[0] is m.factors[userid] and len(m._factors_dev) == 2 + extra
    assert np.array_equal(m.ops.to_host(m._factors_dev[1]), m.factors[userid])
    if extra:
        assert np.array_equal(m.ops.to_host(m._factors_dev[2]), m.factors[f'{itemid}_features'])
    assert m._is_ready and m._factor_image is not None
    m.rank = m.rank + 1
    assert m._is_ready is False and m._factor_image is None


def test_rows_by_norm_is_the_stable_argsort_of_the_row_norms():
    X = np.random.RandomState(5).standard_normal((37, 5))
    X[30] = X[5]                    # two rows of equal norm
    X[20] = 0.
    norms = np.linalg.norm(X, axis=1)
    assert norms[30] == norms[5] and norms[20] == 0.
    m = _small_pmf()
    assert not hasattr(m.ops, 'norm_order')                 # the double: the host statement of HipOps.norm_order
    order, Xs = m._rows_by_norm(m.ops.to_device(X))
    assert isinstance(order, np.ndarray) and order.dtype == np.int64
    assert np.array_equal(order, np.argsort(-norms, kind='stable')) and order[-1] == 20
    assert list(order).index(5) + 1 == list(order).index(30)            # ties by index
    assert np.array_equal(m.ops.to_host(Xs), X[order])
