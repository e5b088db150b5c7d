"""Implicit ALS, host side (no GPU): the confidence transform, the model's surface and refusals, its orchestration on a CPU
double of the device operators (tests/ials_reference.py: IALSNumpyOps) against the NumPy restatement, and the objective."""
import numpy as np
import pytest
import scipy.sparse as sps

import ials_reference as ref
from polara_amd import ials
from polara_amd.models import ScaledMatrixMixin


class ScaledIALS(ScaledMatrixMixin, ials.ImplicitALS):
    pass


def small_data(values=None, holdout=False):
    u = np.array([0, 0, 0, 1, 1, 2, 2, 2, 3, 3])
    i = np.array([0, 2, 3, 1, 2, 0, 1, 4, 3, 4])
    f = np.array([5., 1., 3., 4., 2., 1., 5., 3., 2., 4.]) if values is None else np.asarray(values, dtype=np.float64)
    return ref.model_data(u, i, f, 4, 5, holdout=holdout), (u, i, f)


# ---- confidence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weight', [None, np.log2, np.sqrt])
def test_confidence_is_the_wrappers_expression(weight):
    v = np.array([1., 2., 3.5, 5., 0.25])
    for alpha, epsilon in ((1, 1), (40, 0.5), (0.3, 2)):
        got = ials.ImplicitALS.confidence(v, alpha=alpha, weight=weight, epsilon=epsilon)
        want = (alpha * (weight(v / epsilon) if weight is not None else v / epsilon)).astype('double')
        assert got.dtype == np.float64 and np.array_equal(got, want)
    assert ials.ImplicitALS.confidence(v, dtype='float32').dtype == np.float32
    assert np.array_equal(ials.ImplicitALS.confidence(v), v)              # the defaults of the static method: no weight


def test_zero_confidences_are_dropped():
    data, (u, i, f) = small_data()
    m = ials.ImplicitALS(data, ops=ref.IALSNumpyOps())
    C = m._confidence_csr(m._training_device_csr())
    keep = f != 1.
    want = sps.csr_matrix((np.log2(f[keep]), (u[keep], i[keep])), shape=(4, 5))
    assert C.nnz == keep.sum() == 8 and np.array_equal(C.m.indptr, want.indptr) and np.array_equal(C.m.indices, want.indices)
    assert np.array_equal(C.m.data, want.data) and np.array_equal(C.values.numpy(), want.data)
    m.weight_func = None                                                 # nothing is zero then: the pattern is kept
    C = m._confidence_csr(m._training_device_csr())
    assert C.nnz == 10 and np.array_equal(C.m.data, f)


@pytest.mark.parametrize('values, weight, count', [([5., 1., 3., 4., 0.5, 1., 5., 3., 0.25, 4.], np.log2, 2),
                                                    ([5., 1., 3., 4., 0., 1., 5., 3., 2., 4.], np.log2, 1),
                                                    ([5., 1., 3., -4., 2., 1., 5., 3., 2., 4.], None, 1),
                                                    ([5., 1., 3., -4., 2., 1., 5., 3., 2., 4.], np.sqrt, 1)])
def test_negative_and_non_finite_confidences_raise(values, weight, count):
    data, _ = small_data(values)
    m = ials.ImplicitALS(data, ops=ref.IALSNumpyOps())
    m.verbose, m.weight_func = False, weight
    with pytest.raises(ValueError, match='%d of 10 confidence values' % count):
        m.build()
    assert not m._is_ready and m.factors == {}


# ---- surface ---------------------------------------------------------------------------------------------------------------
def test_exports_and_defaults():
    import polara_amd
    assert 'ImplicitALS' in polara_amd.__all__ and polara_amd.ImplicitALS is ials.ImplicitALS
    m = polara_amd.ImplicitALS(small_data()[0], ops=ref.IALSNumpyOps())
    got = {k: getattr(m, k) for k in ('rank', 'alpha', 'epsilon', 'weight_func', 'regularization', 'num_epochs', 'method', 'num_threads',
                                      'seed', 'compute_loss', 'loss_history', 'iterations_time')}
    assert got == dict(rank=10, alpha=1, epsilon=1, weight_func=np.log2, regularization=0.01, num_epochs=15, method='iALS',
                       num_threads=0, seed=None, compute_loss=False, loss_history=None, iterations_time=None)
    assert m.factors == {}
    m.num_threads = 8                                                    # accepted and ignored
    m.rank, m.num_epochs = 2, 1
    m.verbose = False
    m.build()
    assert m.factors['userid'].shape == (4, 2) and m.factors['itemid'].shape == (5, 2)
    assert not hasattr(polara_amd, 'KernelizedPMF') and not hasattr(polara_amd, 'RandomModel')


def test_initial_factors_follow_the_documented_stream():
    X0, Y0 = ials.initial_factors(5, 4, 3, seed=7)
    rs = np.random.RandomState(7)
    assert np.array_equal(X0, rs.rand(5, 3) * 0.01) and np.array_equal(Y0, rs.rand(4, 3) * 0.01)
    np.random.seed(11)
    X0, Y0 = ials.initial_factors(5, 4, 3)
    rs = np.random.RandomState(11)
    assert np.array_equal(X0, rs.rand(5, 3) * 0.01) and np.array_equal(Y0, rs.rand(4, 3) * 0.01)


def test_a_rank_change_invalidates_the_model():
    case = ref.model_case('r7')
    m = ref.model_for(case, ref.IALSNumpyOps())
    m.num_epochs = 1
    m.build()
    assert m._is_ready and len(m.training_time) == 1
    m.rank = case['rank']
    assert m._is_ready                                                  # the same rank: nothing happens
    m.rank = 4
    assert not m._is_ready and m._recommendations is None and m._factor_image is None
    recs = m.recommendations
    assert len(m.training_time) == 2 and m.factors['userid'].shape[1] == 4 and recs.shape == case['lists'].shape


def test_multi_process_and_bad_ranks_are_refused():
    case = ref.model_case('r7')

    class Counting(ref.IALSNumpyOps):
        calls = 0

        def csr_from_coo(self, *a, **kw):
            Counting.calls += 1
            return super().csr_from_coo(*a, **kw)
    ops = Counting()
    m = ref.model_for(case, ops)
    for rank in (0, -1, ref.MAX_RANK + 1):
        m.rank = rank
        with pytest.raises(ValueError, match='rank %d outside 1..128' % rank):
            m.build()
    assert Counting.calls == 0 and not m._is_ready                       # refused before any work on the matrix
    m.rank = 7

    class Two:
        world, rank = 2, 0
    m.comm = Two()
    with pytest.raises(NotImplementedError, match='multi-process'):
        m.build()
    A = ops.csr_replace_values(ops.csr_from_coo(*case['triplets'], (case['n_users'], case['n_items'])), case['triplets'][2])
    with pytest.raises(NotImplementedError, match='multi-process'):
        ials.ials_fit(ops, A, 7, 0.01, 1, comm=Two())
    with pytest.raises(ValueError, match='rank 129'):
        ials.ials_fit(ops, A, 129, 0.01, 1)
    with pytest.raises(ValueError, match='initial factors'):
        ials.ials_fit(ops, A, 7, 0.01, 1, init=(np.zeros((3, 7)), np.zeros((case['n_items'], 7))))


def test_the_library_states_its_bounds_without_a_device():
    from polara_amd import _lib
    lib = _lib.load()
    assert lib.pk_ials_max_rank() == ref.MAX_RANK == 128
    assert lib.pk_ials_work_bytes(1000, 50) >= 8000 and lib.pk_ials_work_bytes(0, 1) > 0
    rc = lib.pk_ials_half_step_f64(None, 10, 10, 129, None, None, None, None, None, 129, None, 129, 0.01, None, 129, None, None)
    assert rc == -1 and b'rank' in lib.pk_last_error()                   # PK_E_INVALID before anything is enqueued
    rc = lib.pk_ials_loss_nz_f64(None, 10, 10, 0, None, None, None, None, 1, None, 1, None, None)
    assert rc == -1 and b'rank' in lib.pk_last_error()


def test_scaled_composition_passes_the_scaled_values_to_confidence():
    case = ref.model_case('r7')
    seen = []

    def weight(v):
        seen.append(np.array(v))
        return np.log2(v)
    m = ref.model_for(case, ref.IALSNumpyOps(), cls=ScaledIALS)
    assert m.method == 'iALS-s'
    m.weight_func, m.epsilon, m.num_epochs = weight, 0.25, 1
    m.build()
    scaled = m.get_training_matrix()                                    # the mixin's host statement of D_r A D_c
    scaled.sort_indices()
    assert len(seen) == 1 and np.allclose(seen[0], scaled.data / 0.25, rtol=1e-15, atol=0)
    plain = ref.model_for(case, ref.IALSNumpyOps())
    plain.epsilon, plain.num_epochs = 0.25, 1
    plain.build()
    assert ref.rel_distance(m.factors['userid'], plain.factors['userid']) > 1e-3
    assert m.factors['itemid'].shape == plain.factors['itemid'].shape


def test_warm_start_without_filtering_raises():
    w = ref.warm_case('r7')
    m = ref.model_for(w['case'], ref.IALSNumpyOps(), data=ref.warm_data(w))
    m.num_epochs = 1
    m.build()
    m.filter_seen = False
    with pytest.raises(ValueError, match='The model always filters seen items from results.'):
        m.get_recommendations()


# ---- the model on the CPU double --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['r7', 'r16', 'r17'])
def test_model_on_the_cpu_double_gives_the_restatements_lists(name):
    case = ref.model_case(name)
    m = ref.model_for(case, ref.IALSNumpyOps(), compute_loss=True)
    m.build()
    # (the double's Gram product is torch's, the restatement's NumPy's: the same bound as for the device)
    assert max(ref.rel_distance(m.factors['userid'], case['X']), ref.rel_distance(m.factors['itemid'], case['Y'])) <= 16 * case['d']
    assert np.array_equal(m._get_test_data()[2], case['test_users'])
    recs = m.get_recommendations()
    ref.check_lists(recs, case['lists'], case['gaps'])
    assert (case['gaps'] > 1e-9).all()                                   # none left out on these inputs
    assert np.allclose(np.array(m.loss_history), case['loss'], rtol=1e-12, atol=0) and len(m.iterations_time) == case['epochs']
    s, _ = m.slice_recommendations(*m._get_test_data()[:2], 2, 7, m._get_test_data()[2])
    assert np.allclose(s, case['X'][case['test_users'][2:7]] @ case['Y'].T, rtol=0, atol=1e-13)
    assert set(m.factors) == {'userid', 'itemid'} and len(m.training_time) == 1


def test_warm_start_on_the_cpu_double():
    w = ref.warm_case('r7')
    case = w['case']
    m = ref.model_for(case, ref.IALSNumpyOps(), data=ref.warm_data(w))
    m.build()
    assert ref.rel_distance(m.factors['itemid'], case['Y']) <= 16 * case['d']
    tu, ti, tf = w['test']
    keep = tf != 1.
    Cw = sps.csr_matrix((np.log2(tf[keep]), (tu[keep], ti[keep])), shape=(w['n_new'], case['n_items']))
    Cw.sort_indices()
    Y = m.factors['itemid']
    want = ref.half_step(Cw, Y, Y.T @ Y, ref.LAMBDA)
    assert np.allclose(m.fold_in().numpy(), want, rtol=1e-10, atol=1e-14)
    recs = m.get_recommendations()
    lists, gaps = ref.lists_and_gaps(want @ Y.T, (tu, ti))
    ref.check_lists(recs, lists, gaps)
    for u in range(w['n_new']):
        assert not set(recs[u]) & set(ti[tu == u])                      # confidence-0 test items are seen items too


# ---- the objective ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind, rank', [('wide', 50), ('wide', 3), ('narrow', 16), ('tall', 5)])
def test_objective_by_traces_equals_the_dense_one(kind, rank):
    C = ref.confidence_matrix(kind)
    X, Y = ref.item_block(C.shape[0], rank, seed=1), ref.item_block(C.shape[1], rank)
    for lam in (0.01, 1e-6, 3.):
        dense, traces = ref.objective(C, X, Y, lam), ref.objective_by_traces(C, X, Y, lam)
        assert abs(dense - traces) <= 1e-12 * abs(dense)


@pytest.mark.parametrize('name', list(ref.MODEL_CASES))
def test_objective_never_increases_over_a_build(name):
    loss = ref.model_case(name)['loss']
    assert len(loss) == 2 * ref.MODEL_CASES[name][3]
    assert (loss[1:] <= loss[:-1] * (1 + 1e-12)).all() and loss[-1] < loss[0]
    dense = ref.objective(ref.model_case(name)['C'], ref.model_case(name)['X'], ref.model_case(name)['Y'], ref.LAMBDA)
    assert abs(dense - loss[-1]) <= 1e-12 * abs(dense)
