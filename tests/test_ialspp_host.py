"""iALS++, host side (no GPU): the three properties of the block step on the NumPy restatement (tests/ialspp_reference.py) — the
exact block minimum, one block over the rank = exact ALS, exact ALS is a fixed point —, the cached predictions, the margin by
which a lost term misses the tolerance of the device tests, and the model on a CPU double of the device operators.

Measured here (restatement, X0 = 0.1 randn, seed 3): the single-block step stays below 0.0053 of the sum of
`ials_reference.row_bounds` and `step_bounds` against the exact half-step; `np.linalg.solve` in place of the plain Cholesky moves a
step by at most 0.049 of `step_bounds`; the step with the last interaction of every row dropped lies between 2.2e8 and 1.5e9 times outside `step_bounds` over the
cases of tests/test_gpu_ialspp.py (smallest: 'wide', rank 64, d = 64) — DROPPED_MARGIN is a decade below that."""
import numpy as np
import pytest
import scipy.sparse as sps

import ials_reference as ials_ref
import ialspp_reference as ref
from polara_amd import ials, ialspp

DROPPED_MARGIN, STEP_CASES, start = ref.DROPPED_MARGIN, ref.STEP_CASES, ref.start


# ---- the three properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind, rank', [('wide', 5), ('wide', 16), ('wide', 50), ('narrow', 16), ('tall', 5)])
def test_one_block_over_the_rank_is_the_exact_half_step(kind, rank):
    C = ials_ref.confidence_matrix(kind)
    Y = ials_ref.item_block(C.shape[1], rank)
    G = Y.T @ Y
    X0 = start(C, rank)
    X, E0 = X0.copy(), ref.predict(C, X0, Y)
    E = E0.copy()
    ref.block_step(C, Y, X, E, G, 0, 64, 0.01)
    want = ials_ref.half_step(C, Y, G, 0.01)
    # the step solves for x0 - x, the half-step for x: the two differ within the sum of their bounds
    bounds = ials_ref.row_bounds(C, Y, G, 0.01, want) + ref.step_bounds(C, Y, G, 0.01, X0, E0, 0, 64, X)[0]
    err = np.linalg.norm(X - want, axis=1)
    full = bounds > 0
    print('single block %s rank %d: largest error / (row bound + step bound) = %.3g' % (kind, rank, (err[full] / bounds[full]).max()))
    assert (err <= bounds).all() and not X[~full].any()
    assert np.abs(E - ref.predict(C, X, Y)).max() <= 1e-13


@pytest.mark.parametrize('kind, rank, d', [('wide', 5, 16), ('wide', 50, 16), ('wide', 50, 32), ('wide', 160, 64), ('narrow', 16, 16),
                                           ('tall', 5, 16)])
def test_a_block_step_never_increases_the_objective(kind, rank, d):
    C = ials_ref.confidence_matrix(kind)
    Y = ials_ref.item_block(C.shape[1], rank)
    G = Y.T @ Y
    X = start(C, rank)
    values = [ref.objective_terms(C, X, Y, 0.01, 0.01)]
    worst_drift = 0.0
    for _ in range(2):
        _, E = ref.half_sweep(C, Y, X, G, 0.01, d, after_block=lambda p0, X, E: values.append(ref.objective_terms(C, X, Y, 0.01, 0.01)))
        worst_drift = max(worst_drift, np.abs(E - ref.predict(C, X, Y)).max())
    f = np.array([v[0] for v in values])
    slack = np.array([v[2] * ials_ref.EPS * v[1] for v in values])
    assert len(f) == 1 + 2 * -(-rank // d) and f[-1] < f[0]
    print('%s rank %d d %d: largest rise %.3g relative, prediction drift %.3g' % (kind, rank, d, ((f[1:] - f[:-1]) / f[:-1]).max(), worst_drift))
    assert (f[1:] - f[:-1] <= slack[:-1]).all()
    assert worst_drift <= 1e-13                                          # the cached predictions stay those of X


def test_the_exact_solution_is_a_fixed_point_of_every_block():
    C = ials_ref.confidence_matrix('wide')
    rank, d = 50, 16
    Y = ials_ref.item_block(C.shape[1], rank)
    G = Y.T @ Y
    X = ials_ref.half_step(C, Y, G, 0.01)
    E = ref.predict(C, X, Y)
    moved, allowed = np.zeros(C.shape[0]), np.zeros(C.shape[0])
    for p0 in range(0, rank, d):
        X0, E0 = X.copy(), E.copy()
        ref.block_step(C, Y, X, E, G, p0, d, 0.01)
        moved += np.linalg.norm(X - X0, axis=1)
        allowed += ref.step_bounds(C, Y, G, 0.01, X0, E0, p0, d, X)[0]
    assert (moved <= allowed).all() and moved.max() <= 1e-12 * np.linalg.norm(X, axis=1).max()


# ---- the tolerance of the device tests cannot hide a lost term ----------------------------------------------------------------
def test_a_dropped_interaction_lies_far_outside_the_step_bounds():
    smallest, largest_lapack = np.inf, 0.0
    for kind, cases, lams in (('wide', STEP_CASES, (0.01, 1e-6)), ('tall', [(5, 16, 0)], (0.01,)), ('narrow', [(16, 16, 0)], (0.01,))):
        C = ials_ref.confidence_matrix(kind)
        for rank, d, p0 in cases:
            Y = ials_ref.item_block(C.shape[1], rank)
            G = Y.T @ Y
            X0 = start(C, rank)
            E0 = ref.predict(C, X0, Y)
            for lam in lams:
                X1, E1 = X0.copy(), E0.copy()
                ref.block_step(C, Y, X1, E1, G, p0, d, lam)
                X2, E2 = X0.copy(), E0.copy()
                ref.block_step(C, Y, X2, E2, G, p0, d, lam, solve=ials_ref.lapack_solve)
                rows, entries = ref.step_bounds(C, Y, G, lam, X0, E0, p0, d, X1)
                assert (np.linalg.norm(X2 - X1, axis=1) <= rows).all() and (np.abs(E2 - E1) <= entries).all()
                full = rows > 0
                largest_lapack = max(largest_lapack, (np.linalg.norm(X2 - X1, axis=1)[full] / rows[full]).max())
                smallest = min(smallest, ref.dropped_interaction_margin(C, Y, G, lam, X0, E0, p0, d, X1, rows))
    print('dropped interaction: smallest margin %.3g; np.linalg.solve against the Cholesky statement: %.3g of the bound'
          % (smallest, largest_lapack))
    assert smallest >= DROPPED_MARGIN


def test_a_refused_row_is_left_as_it_was():
    C = ials_ref.confidence_matrix('narrow')
    Y = ials_ref.item_block(12, 16)
    Y[:, 12:] = 0.0
    X = start(C, 16)
    E = ref.predict(C, X, Y)
    X0, E0 = X.copy(), E.copy()
    nonempty = np.flatnonzero(np.diff(C.indptr))
    with pytest.raises(ref.NotPositiveDefinite, match=r'%d row\(s\).*first is row %d\b' % (len(nonempty), nonempty[0])):
        ref.block_step(C, Y, X, E, Y.T @ Y, 0, 16, 0.0)
    empty = np.diff(C.indptr) == 0
    assert np.array_equal(X[~empty], X0[~empty]) and not X[empty].any() and np.array_equal(E, E0)


def test_per_row_regularization_is_the_documented_expression():
    C = ials_ref.confidence_matrix('narrow')
    n = np.diff(C.indptr)
    assert ref.row_regularization(C, 0.3) == 0.3 and ref.row_regularization(C, 0.3, 0.0, 5.0) == 0.3
    assert np.array_equal(ref.row_regularization(C, 0.3, 1.0, 2.0), 0.3 * (n + 2.0 * 12))
    assert np.allclose(ref.row_regularization(C, 0.3, 0.5, 1.0), 0.3 * np.sqrt(n + 12.0), rtol=1e-15)
    ops = ref.IALSPPNumpyOps()
    Cd = ops.csr(C.indptr, C.indices, C.data, C.shape)
    assert ialspp.row_regularization(ops, Cd, 0.3) == 0.3
    for nu, a0 in ((1.0, 2.0), (0.5, 1.0)):
        assert np.array_equal(ialspp.row_regularization(ops, Cd, 0.3, nu, a0).numpy(), ref.row_regularization(C, 0.3, nu, a0))
    # a vector of equal values is the scalar path, and the objective by traces is the dense one
    Y = ials_ref.item_block(12, 16)
    X = start(C, 16)
    Xv = X.copy()
    ref.half_sweep(C, Y, X, Y.T @ Y, 0.01, 16)
    ref.half_sweep(C, Y, Xv, Y.T @ Y, np.full(C.shape[0], 0.01), 16)
    assert np.array_equal(X, Xv)
    lr, lc = ref.row_regularization(C, 0.01, 1.0), ref.row_regularization(C.T.tocsr(), 0.01, 1.0)
    dense, traces = ref.objective(C, X, Y, lr, lc), ref.objective_by_traces(C, X, Y, lr, lc)
    assert abs(dense - traces) <= 1e-12 * abs(dense)
    assert abs(ref.objective(C, X, Y, 0.01, 0.01) - ials_ref.objective(C, X, Y, 0.01)) <= 1e-13 * abs(dense)


# ---- surface ---------------------------------------------------------------------------------------------------------------
def test_exports_and_defaults():
    import polara_amd
    assert 'ImplicitALSPP' in polara_amd.__all__ and polara_amd.ImplicitALSPP is ialspp.ImplicitALSPP
    assert issubclass(ialspp.ImplicitALSPP, ials.ImplicitALS)
    m = polara_amd.ImplicitALSPP(ials_ref.model_data(*ials_ref.ratings_matrix(1, 6, 5, 0.6), 6, 5, holdout=False), ops=ref.IALSPPNumpyOps())
    got = {k: getattr(m, k) for k in ('rank', 'regularization', 'num_epochs', 'method', 'block_size', 'reg_exponent', 'reg_unobserved',
                                      'fold_in_sweeps', 'seed', 'compute_loss', 'loss_history')}
    assert got == dict(rank=10, regularization=0.01, num_epochs=15, method='iALS++', block_size=64, reg_exponent=0.0, reg_unobserved=1.0,
                       fold_in_sweeps=8, seed=None, compute_loss=False, loss_history=None)
    m.verbose, m.num_epochs = False, 1
    m.build()
    assert m.factors['userid'].shape == (6, 10) and m.factors['itemid'].shape == (5, 10)


def test_the_library_states_its_bounds_without_a_device():
    from polara_amd import _lib
    lib = _lib.load()
    assert lib.pk_ialspp_max_rank() == ref.MAX_RANK == 2048 and lib.pk_ials_max_rank() == 128
    assert lib.pk_ialspp_work_bytes(1000, 64) >= 4000 and lib.pk_ialspp_work_bytes(0, 16) > 0
    args = (None, None, None, None, None, 4096, None, 4096, 0.01, None, None, 64, None, 4096, None, None, None)
    for rank, p0, d, word in ((2049, 0, 64, b'rank'), (0, 0, 64, b'rank'), (100, 0, 48, b'block size'), (100, 100, 64, b'block start')):
        rc = lib.pk_ialspp_block_step_f64(None, 10, 10, rank, p0, d, *args)
        assert rc == -1 and word in lib.pk_last_error()                  # PK_E_INVALID before anything is enqueued
    rc = lib.pk_ialspp_predict_f64(None, 10, 10, 2049, None, None, None, 4096, None, 4096, None)
    assert rc == -1 and b'rank' in lib.pk_last_error()


def test_bad_block_sizes_ranks_and_multi_process_builds_are_refused():
    case = ref.model_case('r16')
    ops = ref.IALSPPNumpyOps()
    m = ref.model_for(case, ops)
    for d in (0, 8, 48, 128, 16.5):
        m.block_size = d
        with pytest.raises(ValueError, match='block size'):
            m.build()
    m.block_size = 16
    for rank in (0, -1, ref.MAX_RANK + 1):
        m.rank = rank
        with pytest.raises(ValueError, match='rank %d outside 1..2048' % rank):
            m.build()
    assert not m._is_ready
    m.rank = 16

    class Two:
        world, rank = 2, 0
    m.comm = Two()
    with pytest.raises(NotImplementedError, match='multi-process'):
        m.build()
    A = ops.csr_replace_values(ops.csr_from_coo(*case['triplets'], (case['n_users'], case['n_items'])), case['triplets'][2])
    with pytest.raises(NotImplementedError, match='multi-process'):
        ialspp.ialspp_fit(ops, A, 7, 0.01, 1, 16, comm=Two())
    with pytest.raises(ValueError, match='rank 2049'):
        ialspp.ialspp_fit(ops, A, 2049, 0.01, 1, 16)
    with pytest.raises(ValueError, match='block size'):
        ialspp.ialspp_fit(ops, A, 7, 0.01, 1, 24)
    with pytest.raises(ValueError, match='initial factors'):
        ialspp.ialspp_fit(ops, A, 7, 0.01, 1, 16, init=(np.zeros((3, 7)), np.zeros((case['n_items'], 7))))


# ---- the model on the CPU double --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['r16', 'r40'])
def test_model_on_the_cpu_double_gives_the_restatements_lists(name):
    case = ref.model_case(name)
    m = ref.model_for(case, ref.IALSPPNumpyOps(), compute_loss=True)
    m.build()
    assert m.method == 'iALS++'
    assert max(ials_ref.rel_distance(m.factors['userid'], case['X']), ials_ref.rel_distance(m.factors['itemid'], case['Y'])) <= 16 * case['d']
    recs = m.get_recommendations()
    assert (case['gaps'] >= ref.MIN_GAP).all()
    ials_ref.check_lists(recs, case['lists'], case['gaps'], min_gap=0.0, max_left_out=0.0)
    loss = np.array(m.loss_history)
    assert len(loss) == 2 * case['epochs'] and np.allclose(loss, case['loss'], rtol=1e-12, atol=0) and len(m.iterations_time) == case['epochs']
    assert (loss[1:] <= loss[:-1] * (1 + 1e-12)).all()


@pytest.mark.parametrize('name', ['r7', 'r16'])
def test_one_block_is_the_same_fit_as_implicit_als(name):
    case = ials_ref.model_case(name)
    exact = ials_ref.model_for(case, ref.IALSPPNumpyOps(), compute_loss=True)
    exact.build()
    m = ials_ref.model_for(case, ref.IALSPPNumpyOps(), cls=ialspp.ImplicitALSPP, compute_loss=True)
    m.block_size = 16
    m.build()
    dist = max(ials_ref.rel_distance(m.factors[f], exact.factors[f]) for f in ('userid', 'itemid'))
    print('one block against ImplicitALS, %s: distance %.3g (%.2f d)' % (name, dist, dist / case['d']))
    assert dist <= 16 * case['d']
    assert np.allclose(m.loss_history, exact.loss_history, rtol=1e-12, atol=0)
    assert np.array_equal(m.get_recommendations(), exact.get_recommendations())


def test_warm_start_on_the_cpu_double():
    w = ref.warm_case('r16')
    case = w['case']
    m = ref.model_for(case, ref.IALSPPNumpyOps(), data=ials_ref.warm_data(w))
    m.build()
    tu, ti, tf = w['test']
    keep = tf != 1.
    Cw = sps.csr_matrix((np.log2(tf[keep]), (tu[keep], ti[keep])), shape=(w['n_new'], case['n_items']))
    Cw.sort_indices()
    Y = m.factors['itemid']
    G = Y.T @ Y
    assert np.allclose(m.fold_in().numpy(), ref.fold_in(Cw, Y, G, ref.LAMBDA, 16, 8), rtol=1e-10, atol=1e-14)
    # rank 16 in one block: the first sweep is the exact fold-in, the others leave it where it is
    exact = ials_ref.half_step(Cw, Y, G, ref.LAMBDA)
    m.fold_in_sweeps = 1
    assert np.allclose(m.fold_in().numpy(), exact, rtol=1e-10, atol=1e-14)
    recs = m.get_recommendations()
    lists, gaps = ials_ref.lists_and_gaps(exact @ Y.T, (tu, ti))
    ials_ref.check_lists(recs, lists, gaps)
    m.filter_seen = False
    with pytest.raises(ValueError, match='The model always filters seen items from results.'):
        m.get_recommendations()


def test_reg_exponent_reaches_the_solver():
    case = ref.model_case('r40')
    m = ref.model_for(case, ref.IALSPPNumpyOps(), compute_loss=True)
    m.reg_exponent, m.reg_unobserved, m.num_epochs = 1.0, 0.5, 2
    m.build()
    loss = []
    X, Y = ref.fit(case['C'], case['rank'], ref.LAMBDA, 2, case['block'], seed=case['seed'], loss_history=loss, reg_exponent=1.0,
                   reg_unobserved=0.5)
    assert np.allclose(m.factors['userid'], X, rtol=1e-9, atol=1e-13) and np.allclose(m.factors['itemid'], Y, rtol=1e-9, atol=1e-13)
    assert np.allclose(m.loss_history, loss, rtol=1e-12, atol=0)
    assert ials_ref.rel_distance(X, case['X']) > 1e-3                    # and it is another fit than the plain lambda's
