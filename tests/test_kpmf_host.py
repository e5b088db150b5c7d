"""Kernelized PMF, host side (no GPU): the NumPy restatement of the device's sweep (tests/kpmf_reference.py) against the
reference's own fixtures (tests/golden/kpmf_*.npz from tests/golden/make_golden_kpmf.py), what the fixtures can and cannot tell
apart, the kernel matrices, the refusals, and the model's orchestration on a CPU double of the device operators.

Tolerance: every comparison with the reference is at 4 x the fixture's `restatement_gap` — the distance the generator measured
between the restatement and the reference (they differ in rounding alone: the tree of `pm @ qn`, the canonical kernel rows and
the position of the diagonal term in the kernel sum)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import kpmf_reference as ref
from conftest import load_golden
from polara_amd import kpmf, pmf
from test_coldstart_host import EVAL_KEYS
from test_pmf_host import check_against_fixture

FIXTURES = ['kpmf_std', 'kpmf_items_only', 'kpmf_aligned_b4', 'kpmf_adagrad', 'kpmf_rmsprop']
SHORT = ['kpmf_adagrad', 'kpmf_rmsprop']            # three epochs: what the CPU double of the model is driven on


@functools.lru_cache(maxsize=None)
def restated_solution(name):
    """(P, Q, RMSE history) of the restatement on a fixture: computed once, shared with the device tests, never written to"""
    g = load_golden(name)
    out = ref.solve(ref.fixture_plan(g), g['P0'], g['Q0'], **ref.solver_args(g))
    for a in out:
        a.setflags(write=False)
    return out


def same_canonical(A, B):
    A, B = kpmf.canonical_kernel(A), kpmf.canonical_kernel(B)
    return A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) \
        and np.array_equal(A.data, B.data)


def crossing_share(ptr, idx, part):
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return float((part[rows] != part[idx]).mean()) if len(idx) else 0.


# ---- the restatement against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_matches_the_reference(name):
    g = load_golden(name)
    check_against_fixture(g, *restated_solution(name))
    scale = max(np.abs(g['P']).max(), np.abs(g['Q']).max())
    assert float(g['restatement_gap']) <= 1e-12 * scale
    assert float(g['min_rel_gap']) >= 1e-6 and float(g['min_refined_ratio']) >= 1.01


def test_the_fixtures_cover_what_was_asked():
    g = {n: load_golden(n) for n in FIXTURES}
    cfg = lambda n: (int(g[n]['blocks']), int(g[n]['rank']), str(g[n]['adjust']), float(g[n]['learn_rate']), int(g[n]['num_epochs']))
    assert cfg('kpmf_std') == (1, 10, 'none', 0.005, 25) and cfg('kpmf_items_only') == (1, 10, 'none', 0.005, 25)
    assert cfg('kpmf_aligned_b4') == (4, 10, 'none', 0.005, 25)
    assert cfg('kpmf_adagrad') == (1, 10, 'adagrad', 0.05, 3) and cfg('kpmf_rmsprop') == (1, 10, 'rmsprop', 0.05, 3)
    for name, x in g.items():
        assert str(x['model']) == 'KPMF' and tuple(x['train_shape']) == (300, 150) and 4000 <= len(x['train_val']) <= 6000
        key = x['train_idx'][:, 0] * 150 + x['train_idx'][:, 1]
        assert (np.diff(key) > 0).all()                                 # the canonical order is row-major
        assert ('rel_u_val' in x) == (name != 'kpmf_items_only') and 'rel_i_val' in x
        perm, block_ptr = pmf.block_schedule(x['train_idx'][:, 0], x['train_idx'][:, 1], 300, 150, int(x['blocks']))
        assert np.array_equal(perm, x['perm']) and np.array_equal(block_ptr, x['block_ptr'])
    Ku, _ = ref.fixture_kernels(g['kpmf_items_only'])                   # the factor_sigma ** 2 * I path
    assert same_canonical(Ku, float(g['kpmf_items_only']['factor_sigma_user']) ** 2 * sps.eye(300).tocsr())


@pytest.mark.parametrize('name', FIXTURES)
def test_kernels_cross_the_parts_except_in_the_aligned_fixture(name):
    g = load_golden(name)
    plan = ref.fixture_plan(g, blocks=4)
    cross_u = crossing_share(plan['ku_ptr'], plan['ku_idx'], plan['user_part'])
    cross_i = crossing_share(plan['ki_ptr'], plan['ki_idx'], plan['item_part'])
    assert np.isclose(cross_u, float(g['cross_users'])) and np.isclose(cross_i, float(g['cross_items']))       # as the generator saw them
    if name == 'kpmf_aligned_b4':
        assert cross_u == 0. and cross_i == 0. and len(plan['ku_idx']) > 0 and len(plan['ki_idx']) > 0
    else:
        assert cross_i > 0.25 and (cross_u > 0.25 or name == 'kpmf_items_only')
        assert len(plan['ku_idx']) > 0 or name == 'kpmf_items_only'


@functools.lru_cache(maxsize=None)
def std_b4_two_epochs(live):
    g = load_golden('kpmf_std')
    args = dict(ref.solver_args(g), num_epochs=2, tol=0.)
    return ref.solve(ref.fixture_plan(g, blocks=4), g['P0'], g['Q0'], live=live, **args)


def test_live_and_snapshot_reads_can_be_told_apart():
    """on the kpmf_std data at B = 4: reading the block's own neighbour rows from the snapshot instead of live moves P and Q
    by far more than any tolerance used here, so a device sweep that did so would fail the bit-for-bit tests"""
    P, Q, _ = std_b4_two_epochs(True)
    sP, sQ, _ = std_b4_two_epochs(False)
    moved = max(np.abs(P - sP).max(), np.abs(Q - sQ).max())
    assert moved > 1e-9
    g = load_golden('kpmf_aligned_b4')                                  # and the aligned fixture sees it through the reference
    args = dict(ref.solver_args(g), num_epochs=2, tol=0.)
    lP, _, _ = ref.solve(ref.fixture_plan(g), g['P0'], g['Q0'], **args)
    sP, _, _ = ref.solve(ref.fixture_plan(g), g['P0'], g['Q0'], live=False, **args)
    assert np.abs(lP - sP).max() > 1e-9


@pytest.mark.parametrize('adjust', [None, 'rmsprop'])
def test_the_cached_user_sum_gives_the_same_bits(adjust):
    g = load_golden('kpmf_std')
    plan = ref.fixture_plan(g, blocks=4)
    assert (np.diff(plan['users']) == 0).sum() > 1000                   # runs of one user exist
    out = []
    for cache in (True, False):
        P, Q = g['P0'].copy(), g['Q0'].copy()
        S = (np.zeros_like(P), np.zeros_like(Q)) if adjust else None
        sse = ref.epoch(plan, P, Q, 0.05, 0.5, adjust, S, cache=cache)
        out.append((P, Q, sse))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def half_identity_kernels(n_users, n_items):
    """Ku = Ki = I / 2: the diagonal is stored and nothing else, so the kernelized term (+0.0 + 0.5 * (p + p)) is p exactly"""
    return 0.5 * sps.identity(n_users, format='csr'), 0.5 * sps.identity(n_items, format='csr')


@pytest.mark.parametrize('adjust', [None, 'adagrad', 'rmsprop'])
def test_half_identity_kernels_give_the_plain_sweep(adjust):
    """the two restatements against each other on a 40 x 25 random matrix: with both kernel matrices I / 2 the kernelized
    epoch leaves P, Q, the state and the squared error bit-equal to the PMF epoch on the same plan, and snapshots equal to P, Q"""
    import pmf_reference
    rng = np.random.RandomState(5)
    dense = rng.rand(40, 25) < 0.3
    u, i = np.nonzero(dense)
    v = rng.randint(1, 6, size=len(u)).astype(np.float64)
    for blocks in (1, 4):
        plan = ref.make_plan(u, i, v, 40, 25, blocks, *half_identity_kernels(40, 25))
        assert plan['ku_idx'].size == 0 and plan['ki_idx'].size == 0 and (plan['ku_diag'] == 0.5).all() and (plan['ki_diag'] == 0.5).all()
        for rank in (3, 17):
            P0, Q0 = rng.normal(scale=0.1, size=(40, rank)), rng.normal(scale=0.1, size=(25, rank))
            out = []
            for epoch in (pmf_reference.epoch, ref.epoch):
                P, Q = P0.copy(), Q0.copy()
                S = (np.zeros_like(P), np.zeros_like(Q))
                snaps = []
                kw = dict(snapshots=snaps) if epoch is ref.epoch else {}
                out.append((P, Q, S[0], S[1], np.float64(epoch(plan, P, Q, 0.05, 0.5, adjust, S if adjust else None, **kw))))
            assert all(np.array_equal(a, b) for a, b in zip(*out)), (blocks, rank)
            assert np.array_equal(snaps[0], out[1][0]) and np.array_equal(snaps[1], out[1][1])
            assert not np.array_equal(out[1][0], P0)


def test_one_epoch_is_the_serial_sweep_with_snapshots():
    """the restated epoch (sample t of all blocks of a stratum at once) against a plain loop over the schedule, block after
    block, that spells the per-sample arithmetic of include/polara_hip.h out entry by entry: bit for bit"""
    g = load_golden('kpmf_std')
    rng = np.random.RandomState(3)
    for blocks, rank, adjust in ((1, 5, None), (4, 10, 'adagrad'), (7, 17, 'rmsprop')):
        plan = ref.fixture_plan(g, blocks=blocks)
        n_users, n_items = plan['shape']
        P0, Q0 = rng.normal(scale=0.1, size=(n_users, rank)), rng.normal(scale=0.1, size=(n_items, rank))
        P, Q = P0.copy(), Q0.copy()
        S = (np.zeros_like(P), np.zeros_like(Q)) if adjust else None
        got = ref.epoch(plan, P, Q, 0.05, 0.5, adjust, S)
        sP, sQ = P0.copy(), Q0.copy()
        sS = (np.zeros_like(P), np.zeros_like(Q))
        w = ref.group_width(rank)
        block_sse = np.zeros(blocks * blocks)

        def off(side, part, mine, X, snap, r):
            acc = np.zeros(rank)
            for e in range(plan[side + '_ptr'][r], plan[side + '_ptr'][r + 1]):
                j = plan[side + '_idx'][e]
                acc = acc + plan[side + '_val'][e] * (X[j] if part[j] == mine else snap[j])
            return acc
        for s in range(blocks):
            snapP, snapQ = sP.copy(), sQ.copy()
            for b in range(blocks):
                for t in range(plan['block_ptr'][s * blocks + b], plan['block_ptr'][s * blocks + b + 1]):
                    m, n, val = plan['users'][t], plan['items'][t], plan['vals'][t]
                    pm, qn = sP[m].copy(), sQ[n].copy()
                    err = val - ref.tree_dot(pm[None], qn[None], w)[0]
                    kp = off('ku', plan['user_part'], b, sP, snapP, m) + plan['ku_diag'][m] * (pm + pm)
                    kq = off('ki', plan['item_part'], (b + s) % blocks, sQ, snapQ, n) + plan['ki_diag'][n] * (qn + qn)
                    gp = err * qn - kp * (0.5 / plan['row_nnz'][m])
                    gq = err * pm - kq * (0.5 / plan['col_nnz'][n])
                    sP[m] = pm + 0.05 * ref.adjusted(adjust, gp[None], sS[0], [m], ref.GAMMA, ref.SMOOTHING)[0]
                    sQ[n] = qn + 0.05 * ref.adjusted(adjust, gq[None], sS[1], [n], ref.GAMMA, ref.SMOOTHING)[0]
                    block_sse[s * blocks + b] += err * err
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


def test_split_kernel_makes_the_matrix_canonical():
    K = sps.csr_matrix((np.array([1., 2., 3., 4., 5., 6.]), np.array([2, 0, 2, 1, 0, 2]), np.array([0, 3, 4, 4, 6])), shape=(4, 4))
    ptr, idx, val, diag = kpmf.split_kernel(K)                          # row 0: unsorted with a duplicate; row 2: empty
    assert ptr.dtype == np.int64 and idx.dtype == np.int32 and val.dtype == diag.dtype == np.float64
    assert ptr.tolist() == [0, 1, 1, 1, 3] and idx.tolist() == [2, 0, 2] and val.tolist() == [4., 5., 6.]
    assert diag.tolist() == [2., 4., 0., 0.]
    assert K.indices.tolist() == [2, 0, 2, 1, 0, 2]                     # the caller's matrix is not written
    with pytest.raises(ValueError, match='kernel matrix of shape'):
        kpmf.split_kernel(K, 5)
    with pytest.raises(ValueError, match='kernel matrix of shape'):
        kpmf.split_kernel(sps.csr_matrix((3, 4)))


# ---- the model on the CPU double ------------------------------------------------------------------------------------------
def check_kpmf_model_against_fixture(m, g, build_kwargs=None):
    """method name, factor keys, kernels, factors, history, stopping epoch, scores, lists, evaluate() — shared with the device tests"""
    adjust = ref.adjust_of(g)
    m.build(**({'adjust_gradient': adjust} if build_kwargs is None else build_kwargs))
    userid, itemid = m.data.fields.userid, m.data.fields.itemid
    assert m.method == str(g['model']) == 'KPMF' and set(m.factors) == {userid, itemid}
    Ku, Ki = ref.fixture_kernels(g)
    assert same_canonical(m.user_kernel_matrix, Ku) and same_canonical(m.item_kernel_matrix, Ki)
    n = g['scores'].shape[0]
    test_data, shape, users = m._get_test_data()
    assert np.array_equal(users, g['test_users'])
    s, _ = m.slice_recommendations(test_data, shape, 0, n, users)
    recs = m.get_recommendations()
    assert recs.dtype == np.int64
    check_against_fixture(g, m.factors[userid], m.factors[itemid], np.array(m.rmse_history), s, recs)
    B = int(g['blocks'])
    assert m.build_stats['blocks'] == m.build_stats['strata'] == B
    assert m.build_stats['empty_blocks'] == int(g['empty_blocks']) and m.build_stats['longest_block'] == int(g['longest_block'])
    assert m.build_stats['epochs'] == len(g['rmse_history']) == len(m.iterations_time)
    scores = {type(x).__name__: x for x in m.evaluate('all')}
    for key in EVAL_KEYS:
        _, family, field = key.split('_', 2)
        assert np.isclose(getattr(scores[family], field), float(g[key]), rtol=1e-12, atol=0), key


@pytest.mark.parametrize('name', SHORT)
def test_model_on_the_cpu_double(name):
    g = load_golden(name)
    m = ref.model_for(g, ref.KPMFNumpyOps())
    check_kpmf_model_against_fixture(m, g)
    P, Q, history = restated_solution(name)                             # the same arithmetic: the same bits
    assert np.array_equal(m.factors['userid'], P) and np.array_equal(m.factors['itemid'], Q)
    assert np.array_equal(np.array(m.rmse_history), history)


@pytest.mark.parametrize('name', FIXTURES)
def test_kernel_matrices_equal_the_recorded_ones(name):
    g = load_golden(name)
    m = ref.model_for(g, ref.KPMFNumpyOps())
    Ku, Ki = ref.fixture_kernels(g)
    assert same_canonical(m.user_kernel_matrix, Ku) and same_canonical(m.item_kernel_matrix, Ki)
    assert m.get_kernel_matrix('userid') is m.user_kernel_matrix and m.get_kernel_matrix('itemid') is m.item_kernel_matrix


def test_exports_and_defaults():
    import polara_amd
    import polara_amd.kpmf
    assert polara_amd.kpmf is kpmf                                      # the model's home: polara_amd.kpmf.KernelizedPMF
    assert kpmf.KernelizedPMF.__mro__[1:3] == (kpmf.KernelizedRecommenderMixin, pmf.ProbabilisticMF)
    m = kpmf.KernelizedPMF(ref.golden_data(load_golden('kpmf_adagrad')), ops=ref.KPMFNumpyOps())
    got = {k: getattr(m, k) for k in ('kernel_type', 'beta', 'gamma', 'sigma', 'kernel_update', 'sparse_kernel_format', 'factor_sigma',
                                      'method', 'seed', 'learn_rate', 'num_epochs', 'rank', 'tolerance', 'blocks')}
    assert got == dict(kernel_type='reg', beta=0.01, gamma=0.1, sigma=1, kernel_update=None, sparse_kernel_format=True,
                       factor_sigma={'userid': 1, 'itemid': 1}, method='KPMF', seed=None, learn_rate=0.005, num_epochs=25, rank=10,
                       tolerance=1e-4, blocks=None)
    assert m.optimizer is kpmf.kernelized_pmf_sgd and m.factors == {}
    assert kpmf.default_blocks(20_000_000, 138_493, 26_744) == pmf.default_blocks(20_000_000, 138_493, 26_744)
    assert 'NOT measured' in kpmf.default_blocks.__doc__
    from polara_amd import machine_model
    assert not any(k.startswith('kpmf') for k in machine_model.MI355X)   # an entry is added only from a measured value


def test_the_data_change_event_clears_the_kernels():
    g = load_golden('kpmf_adagrad')
    m = ref.model_for(g, ref.KPMFNumpyOps())
    Ku = m.user_kernel_matrix
    assert m._kernel_matrices['userid'] is Ku and m._kernel_matrices['itemid'] is None
    m.data._notify(m.data.on_change_event)
    assert m._kernel_matrices == {'userid': None, 'itemid': None}
    m.gamma = 0.2
    assert not same_canonical(m.user_kernel_matrix, Ku)                 # rebuilt, with what the model holds now


# ---- what is refused, before any work ----------------------------------------------------------------------------------
class NoWork(ref.KPMFNumpyOps):
    def kpmf_plan(self, *a, **kw):
        raise AssertionError('work was started')
    csr_from_coo = pmf_plan = kpmf_epoch = kpmf_plan


def refusing_model():
    return ref.model_for(load_golden('kpmf_adagrad'), NoWork())


def test_the_diffusion_kernel_is_refused():
    m = refusing_model()
    m.kernel_type = 'dif'
    with pytest.raises(NotImplementedError, match="kernel_type='dif'"):
        m.build()
    with pytest.raises(NotImplementedError, match="kernel_type='dif'"):
        m.user_kernel_matrix
    m.kernel_type = 'other'
    with pytest.raises(ValueError, match="'other'"):
        m.build()
    assert not m._is_ready and m.factors == {}


def test_dense_kernels_and_a_kernel_update_callable_are_refused():
    m = refusing_model()
    m.sparse_kernel_format = False
    with pytest.raises(NotImplementedError, match='sparse_kernel_format=False'):
        m.build()
    m.sparse_kernel_format = True

    def sp_kernel_update(pm, P, m, K):
        raise AssertionError
    m.kernel_update = sp_kernel_update
    with pytest.raises(NotImplementedError, match='sp_kernel_update'):
        m.build()
    ops = ref.KPMFNumpyOps()
    g = load_golden('kpmf_adagrad')
    A = ops.csr_from_coo(g['train_idx'][:, 0], g['train_idx'][:, 1], g['train_val'], g['train_shape'])
    with pytest.raises(NotImplementedError, match='sp_kernel_update'):
        kpmf.kernelized_pmf_sgd(NoWork(), A, 10, 0.005, 1, 2, 1e-4, ref.fixture_kernels(g), kernel_update=sp_kernel_update)
    with pytest.raises(NotImplementedError, match='sparse_kernel_format=False'):
        kpmf.kernelized_pmf_sgd(NoWork(), A, 10, 0.005, 1, 2, 1e-4, ref.fixture_kernels(g), sparse_kernel_format=False)


@pytest.mark.parametrize('asked', ['adam', 'adanorm', 'gnprop', 'gnpropz', 'something'])
def test_other_adjustments_are_refused_by_name(asked):
    m = refusing_model()

    def fn(*a):
        raise AssertionError
    fn.__name__ = asked
    for arg in (asked, fn):
        with pytest.raises(NotImplementedError, match='KPMF.*' + asked):
            m.build(adjust_gradient=arg)
    assert not m._is_ready and m.factors == {}


def test_warm_start_multi_process_and_plain_data_are_refused():
    m = refusing_model()
    m.data.warm_start = True
    with pytest.raises(NotImplementedError, match='warm start'):
        m.build()
    m.data.warm_start = False

    class Two:
        world, rank = 2, 0
    m.comm = Two()
    with pytest.raises(NotImplementedError, match='multi-process'):
        m.build()
    ops = ref.KPMFNumpyOps()
    g = load_golden('kpmf_adagrad')
    A = ops.csr_from_coo(g['train_idx'][:, 0], g['train_idx'][:, 1], g['train_val'], g['train_shape'])
    with pytest.raises(NotImplementedError, match='multi-process'):
        kpmf.kernelized_pmf_sgd(NoWork(), A, 10, 0.005, 1, 2, 1e-4, ref.fixture_kernels(g), comm=Two())
    import pmf_reference
    plain = kpmf.KernelizedPMF(pmf_reference.golden_data(load_golden('pmf_b4')), ops=NoWork())
    with pytest.raises(NotImplementedError, match='get_relations_matrix'):
        plain.build()

    def simple_pmf_sgd(*a, **kw):
        raise AssertionError
    m = refusing_model()
    m.optimizer = simple_pmf_sgd
    with pytest.raises(NotImplementedError, match='simple_pmf_sgd.*kpmf.kernelized_pmf_sgd'):
        m.build()


def test_the_library_checks_its_arguments_without_a_device():
    from polara_amd import _lib
    lib = _lib.load()

    def call(blocks, rank, n_users=8, n_items=8):
        return lib.pk_kpmf_epoch_f64(None, blocks, rank, 0, n_users, n_items, *([None] * 4), None, 0, None, 0, *([None] * 12), None, 0,
                                     None, 0, 0.1, 0.5, 0, None, 0, None, 0, 0.9, 1e-6, None, None)
    assert call(1, ref.MAX_RANK + 1) == -1 and b'rank' in lib.pk_last_error()          # PK_E_INVALID
    assert call(_lib.PK_PMF_MAX_BLOCKS + 1, 10) == -1 and b'blocks' in lib.pk_last_error()
    assert call(1, 10, n_users=0) == -1 and b'sizes' in lib.pk_last_error()
    assert call(1, 10) == -1 and b'pointers' in lib.pk_last_error()
