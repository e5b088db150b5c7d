"""Logistic matrix factorisation, host side (no GPU): the draw stream, the restated half-step (tests/lmf_reference.py) against a
plain Python loop and against an independent np.longdouble evaluation, what a half-step leaves untouched, the fit on a planted
matrix, the model's surface, refusals and orchestration on a CPU double of the device operators (LMFNumpyOps)."""
import numpy as np
import pytest
import scipy.sparse as sps

import lmf_reference as ref
from polara_amd import lmf
from polara_amd.models import ScaledMatrixMixin

# the smallest, over the rows of the three 'wide' cases below, of the largest |x(one sample dropped) - x| / bound of the row:
# measured 5.5e7 (a positive dropped) and 1.3e8 (a negative dropped) when the test was written; asserted at 1e7, far above the
# 1e3 below which the inputs would have to change
LOST_TERM_MARGIN = 1e7


class ScaledLMF(ScaledMatrixMixin, lmf.ImplicitLMF):
    pass


def small_data(values=None, holdout=False):
    u = np.array([0, 0, 0, 1, 1, 2, 2, 2, 3, 3])
    i = np.array([0, 2, 3, 1, 2, 0, 1, 4, 3, 4])
    f = np.array([5., 1., 3., 4., 2., 1., 5., 3., 2., 4.]) if values is None else np.asarray(values, dtype=np.float64)
    return ref.model_data(u, i, f, 4, 5, holdout=holdout), (u, i, f)


# ---- the draws -----------------------------------------------------------------------------------------------------------------
def test_draws_are_in_range_and_equal_the_naive_loop():
    for seed, rnd, start, m, n_other in ((0, 0, 0, 500, 7), (2 ** 32 - 1, 5, 2 ** 40, 300, 1100), (77, ref.FOLD_IN_ROUND | 3, 123, 64, 1),
                                         (9, 1, 2 ** 63, 200, 2 ** 31 - 1)):
        key = ref.stream_key(seed, rnd)
        got = ref.draws(key, start, m, n_other)
        assert got.dtype == np.int64 and got.shape == (m,) and got.min() >= 0 and got.max() < n_other
        assert np.array_equal(got, ref.naive_draws(key, start, m, n_other))
    assert len(np.unique(ref.draws(ref.stream_key(1, 0), 0, 4000, 1000))) > 950        # uniform over all columns
    assert not np.array_equal(ref.draws(ref.stream_key(1, 0), 0, 50, 1000), ref.draws(ref.stream_key(1, 1), 0, 50, 1000))


def test_negatives_of_a_matrix_follow_the_prefix_sum_and_the_cap():
    C = ref.confidence_matrix('wide')
    lengths = np.diff(C.indptr)
    assert list(lengths[:len(ref.WIDE_LENGTHS)]) == ref.WIDE_LENGTHS and C.shape == (40, 1100)
    ptr = ref.neg_pointers(C.indptr, 1100, 3)
    capped = np.flatnonzero(np.diff(ptr) != 3 * lengths)
    assert list(capped) == [ref.WIDE_LENGTHS.index(1000)] and np.diff(ptr)[capped[0]] == 1100      # the cap binds there alone
    neg = ref.draw_negatives(C, 3, 5, 2)
    assert neg.dtype == np.int32 and len(neg) == ptr[-1]
    key = ref.stream_key(5, 2)
    for u in (1, 7, 20, 39):
        assert np.array_equal(neg[ptr[u]:ptr[u + 1]], ref.naive_draws(key, ptr[u], ptr[u + 1] - ptr[u], 1100))
    # the row's own entries are not excluded: the long row draws some of its own columns
    u = capped[0]
    assert np.isin(neg[ptr[u]:ptr[u + 1]], C.indices[C.indptr[u]:C.indptr[u + 1]]).sum() > 500


# ---- the half-step ---------------------------------------------------------------------------------------------------------
def test_one_chain_equals_a_plain_python_loop_bit_for_bit():
    rng = np.random.RandomState(3)
    dense = (rng.rand(12, 30) < 0.2) * ref.CONFIDENCES[rng.randint(6, size=(12, 30))]
    dense[4] = 0.0
    C = sps.csr_matrix(dense)
    for side in ('user', 'item'):
        X, A, Y, pinned = ref.blocks(12, 30, 3, side)
        got = ref.half_step(C, Y, X, A, 1.0, 0.6, 2, 11, 4, pinned, chains=1)
        want = ref.half_step(C, Y, X, A, 1.0, 0.6, 2, 11, 4, pinned, step=ref.plain_row_step)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes()
        four = ref.half_step(C, Y, X, A, 1.0, 0.6, 2, 11, 4, pinned, chains=4)
        assert four[0].tobytes() != got[0].tobytes() and np.allclose(four[0], got[0], rtol=1e-12, atol=0)      # the chains are real


@pytest.mark.parametrize('rank, neg_prop, side', [(3, 3, 'user'), (30, 1, 'item'), (126, 3, 'user')])
def test_restatement_against_longdouble(rank, neg_prop, side):
    """The restated half-step against an independent evaluation in np.longdouble (80-bit where the platform has it: eps
    5.4e-20; plain dot products and sums, exp of the extended type), within the first-order bound of
    lmf_reference.half_step_bounds.  With eps = 2^-53, T samples in the row's list and K columns:
      * a serial dot product of K terms is off by at most K eps sum |x_c y_qc| (Higham, gamma_K to first order);
      * sigm(s^) against sigm(s): |d log sigm(s) / ds| = 1 - sigm(s) <= 1, so a RELATIVE error of at most |s^ - s|, plus the
        restated sigmoid's own relative error, measured at 2.98e-16 in test_bpr_host.py, plus one rounding for c * sigm;
      * D_c: each term g_q y_qc carries g's relative error and one rounding; a chain adds ceil(T / PK_LMF_CHAINS) terms and the
        chains' sum PK_LMF_CHAINS more: at most (ceil(T / chains) + chains) eps sum |g_q y_qc| to first order;
      * d = D - reg x: two more roundings; a = A + d^2: 2 |d| dd plus two roundings; h = lr / sqrt(1e-6 + a): half the relative
        error of the sum under the root, plus three roundings; x + h d: h dd + |d| dh plus two roundings.
    Everything is doubled for the second-order terms and the reference's own error.  The same test asserts that a half-step that
    loses one positive, or one negative, of a row lands at least LOST_TERM_MARGIN times outside the bound on that row."""
    C = ref.confidence_matrix('wide')
    X, A, Y, pinned = ref.blocks(C.shape[0], C.shape[1], rank, side)
    args = (C, Y, X, A, 1.0, 0.6, neg_prop, 7, 3, pinned)
    got_x, got_a = ref.half_step(*args)
    want_x, want_a, BX, BA = ref.half_step_longdouble(*args)
    assert np.finfo(np.longdouble).eps < 1e-18                           # an extended type: the reference is worth its name
    rows = np.diff(C.indptr) > 0
    moved = np.arange(rank + 2) != pinned
    ex, ea = np.abs(got_x - want_x).astype(np.float64), np.abs(got_a - want_a).astype(np.float64)
    print('largest error / bound: x %.3g, a %.3g' % ((ex[rows][:, moved] / BX[rows][:, moved]).max(), (ea[rows][:, moved] / BA[rows][:, moved]).max()))
    assert (BX[rows][:, moved] > 0).all() and (BA[rows][:, moved] > 0).all()
    assert (ex <= BX).all() and (ea <= BA).all()
    for drop in ('positive', 'negative'):
        lost_x, _ = ref.half_step(*args, drop=drop)
        ratio = (np.abs(lost_x - want_x).astype(np.float64)[rows][:, moved] / BX[rows][:, moved]).max(axis=1)
        print('one %s dropped: smallest row margin %.3g' % (drop, ratio.min()))
        assert ratio.min() >= LOST_TERM_MARGIN


def test_pinned_column_empty_rows_and_their_state_stay_untouched():
    C = ref.confidence_matrix('wide')
    empty = np.diff(C.indptr) == 0
    assert empty.sum() >= 1
    for side in ('user', 'item'):
        X, A, Y, pinned = ref.blocks(C.shape[0], C.shape[1], 5, side)
        X1, A1 = ref.half_step(C, Y, X, A, 1.0, 0.6, 3, 1, 0, pinned)
        assert np.array_equal(X1[:, pinned], X[:, pinned]) and np.array_equal(A1[:, pinned], A[:, pinned])
        assert np.array_equal(X1[empty], X[empty]) and np.array_equal(A1[empty], A[empty])
        others = np.arange(7) != pinned
        assert (X1[~empty][:, others] != X[~empty][:, others]).all() and (A1[~empty][:, others] > A[~empty][:, others]).all()
    # a NaN is not refused: it propagates through its row and stays there
    X, A, Y, pinned = ref.blocks(C.shape[0], C.shape[1], 5, 'user')
    Y[C.indices[C.indptr[3]]] = np.nan
    X1, _ = ref.half_step(C, Y, X, A, 1.0, 0.6, 3, 1, 0, pinned)
    assert np.isnan(X1[3][:6]).all() and X1[3][6] == 1.0 and np.isfinite(X1[1]).all()


def test_fit_ranks_the_planted_block_first():
    dense, ug, ig = ref.planted_matrix()
    X, Y = ref.fit(sps.csr_matrix(dense), 4, 1.0, 0.6, 5, 6, seed=1)
    scores = X @ Y.T
    scores[dense > 0] = -np.inf
    top = np.argsort(-scores, axis=1)[:, :5]
    share = (ig[top] == ug[:, None]).mean()
    print('unseen items of the own block among the top 5: %.3f' % share)
    assert share >= 0.95
    assert (X[:, 5] == 1).all() and (Y[:, 4] == 1).all() and X[:, 4].any() and Y[:, 5].any()       # pinned ones, moved biases


# ---- surface ---------------------------------------------------------------------------------------------------------------
def test_exports_and_defaults():
    import polara_amd
    assert 'ImplicitLMF' in polara_amd.__all__ and polara_amd.ImplicitLMF is lmf.ImplicitLMF
    m = polara_amd.ImplicitLMF(small_data()[0], ops=ref.LMFNumpyOps())
    got = {k: getattr(m, k) for k in ('rank', 'alpha', 'epsilon', 'weight_func', 'learning_rate', 'regularization', 'neg_prop', 'num_epochs',
                                      'fold_in_epochs', 'method', 'num_threads', 'show_progress', 'seed', 'iterations_time', 'build_stats')}
    assert got == dict(rank=30, alpha=1, epsilon=1, weight_func=np.log2, learning_rate=1.0, regularization=0.6, neg_prop=30, num_epochs=30,
                       fold_in_epochs=10, method='LMF', num_threads=0, show_progress=False, seed=None, iterations_time=None,
                       build_stats={})
    assert m.factors == {}
    m.num_threads, m.show_progress = 8, True                            # accepted and ignored
    m.rank, m.num_epochs = 2, 1
    m.verbose = False
    np.random.seed(5)
    m.build()
    assert m.factors['userid'].shape == (4, 4) and m.factors['itemid'].shape == (5, 4)
    assert m.factors['userid'].dtype == m.factors['itemid'].dtype == np.float64
    np.random.seed(5)
    drawn = int(np.random.randint(0, 2 ** 32, dtype=np.uint64))
    # 8 confidences survive log2: min(5, 30 n) and min(4, 30 n) negatives per row
    assert m.build_stats == dict(seed=drawn, epochs=1, neg_prop=30, user_negatives=4 * 5, item_negatives=5 * 4)
    assert len(m.iterations_time) == 1


def test_initial_factors_follow_the_documented_stream():
    X0, Y0 = lmf.initial_factors(5, 4, 3, seed=7)
    rs = np.random.RandomState(7)
    assert np.array_equal(X0[:, :3], rs.normal(scale=0.1, size=(5, 3))) and np.array_equal(Y0[:, :3], rs.normal(scale=0.1, size=(4, 3)))
    assert not X0[:, 3].any() and (X0[:, 4] == 1).all() and (Y0[:, 3] == 1).all() and not Y0[:, 4].any()
    np.random.seed(11)
    X0, _ = lmf.initial_factors(5, 4, 3)
    assert np.array_equal(X0[:, :3], np.random.RandomState(11).normal(scale=0.1, size=(5, 3)))


def test_a_rank_change_invalidates_the_model():
    case = ref.model_case('r5')
    m = ref.model_for(case, ref.LMFNumpyOps())
    m.num_epochs = 1
    m.build()
    assert m._is_ready and len(m.training_time) == 1
    m.rank = case['rank']
    assert m._is_ready
    m.rank = 4
    assert not m._is_ready and m._recommendations is None
    recs = m.recommendations
    assert len(m.training_time) == 2 and m.factors['userid'].shape[1] == 6 and recs.shape == case['lists'].shape


def test_refusals():
    case = ref.model_case('r5')

    class Counting(ref.LMFNumpyOps):
        calls = 0

        def csr_from_coo(self, *a, **kw):
            Counting.calls += 1
            return super().csr_from_coo(*a, **kw)
    ops = Counting()
    m = ref.model_for(case, ops)
    for rank in (0, -1, ref.MAX_RANK + 1):
        m.rank = rank
        with pytest.raises(ValueError, match='rank %d outside 1..126' % rank):
            m.build()
    m.rank = 5
    for neg_prop in (0, -3):
        m.neg_prop = neg_prop
        with pytest.raises(ValueError, match='neg_prop %d < 1' % neg_prop):
            m.build()
    assert Counting.calls == 0 and not m._is_ready                       # refused before any work on the matrix
    m.neg_prop = 2

    class Two:
        world, rank = 2, 0
    m.comm = Two()
    with pytest.raises(NotImplementedError, match='multi-process'):
        m.build()
    A = ops.csr_replace_values(ops.csr_from_coo(*case['triplets'], (case['n_users'], case['n_items'])), case['triplets'][2])
    with pytest.raises(NotImplementedError, match='multi-process'):
        lmf.lmf_fit(ops, A, 5, 1.0, 0.6, 2, 1, comm=Two())
    with pytest.raises(ValueError, match='rank 127'):
        lmf.lmf_fit(ops, A, 127, 1.0, 0.6, 2, 1)
    with pytest.raises(ValueError, match='neg_prop 0'):
        lmf.lmf_fit(ops, A, 5, 1.0, 0.6, 0, 1)
    with pytest.raises(ValueError, match='seed'):
        lmf.lmf_fit(ops, A, 5, 1.0, 0.6, 2, 1, seed=2 ** 32)
    with pytest.raises(ValueError, match='initial factors'):
        lmf.lmf_fit(ops, A, 5, 1.0, 0.6, 2, 1, init=(np.zeros((3, 7)), np.zeros((case['n_items'], 7))))


@pytest.mark.parametrize('values, weight, count', [([5., 1., 3., 4., 0.5, 1., 5., 3., 0.25, 4.], np.log2, 2),
                                                    ([5., 1., 3., 4., 0., 1., 5., 3., 2., 4.], np.log2, 1),
                                                    ([5., 1., 3., -4., 2., 1., 5., 3., 2., 4.], None, 1)])
def test_negative_and_non_finite_confidences_raise(values, weight, count):
    data, _ = small_data(values)
    m = lmf.ImplicitLMF(data, ops=ref.LMFNumpyOps())
    m.verbose, m.weight_func = False, weight
    with pytest.raises(ValueError, match='LMF: %d of 10 confidence values' % count):
        m.build()
    assert not m._is_ready and m.factors == {}


def test_warm_start_without_filtering_raises():
    w = ref.warm_case('r5')
    m = ref.model_for(w['case'], ref.LMFNumpyOps(), data=ref.warm_data(w))
    m.num_epochs = 1
    m.build()
    m.filter_seen = False
    with pytest.raises(ValueError, match='The model always filters seen items from results.'):
        m.get_recommendations()


def test_the_library_states_its_bounds_without_a_device():
    from polara_amd import _lib
    lib = _lib.load()
    assert lib.pk_lmf_max_rank() == ref.MAX_RANK == 126 and lib.pk_lmf_chains() == ref.CHAINS
    args = (None, None, None, None, None, 1, 0, 4, 3, None, 129, 1.0, 0.6, None, 129, None, 129)
    assert lib.pk_lmf_half_step_f64(None, 10, 10, 129, *args) == -1 and b'129 columns' in lib.pk_last_error()
    args = (None, None, None, None, None, 1, 0, 4, 0, None, 8, 1.0, 0.6, None, 8, None, 8)
    assert lib.pk_lmf_half_step_f64(None, 10, 10, 8, *args) == -1 and b'neg_prop' in lib.pk_last_error()
    assert lib.pk_lmf_draw_negatives(None, 10, 10, None, None, 0, 1, 0, None) == -1 and b'neg_prop' in lib.pk_last_error()


# ---- the model on the CPU double --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['r5', 'r14'])
def test_model_on_the_cpu_double_gives_the_restated_fit(name):
    case = ref.model_case(name)
    m = ref.model_for(case, ref.LMFNumpyOps())
    m.build()
    assert m.factors['userid'].tobytes() == case['X'].tobytes() and m.factors['itemid'].tobytes() == case['Y'].tobytes()
    assert set(m.factors) == {'userid', 'itemid'} and len(m.training_time) == 1 and len(m.iterations_time) == case['epochs']
    assert m.build_stats['seed'] == case['seed'] and m.build_stats['epochs'] == case['epochs']
    assert np.array_equal(m._get_test_data()[2], case['test_users'])
    recs = m.get_recommendations()
    ref.check_lists(recs, case['lists'], case['gaps'])
    s, _ = m.slice_recommendations(*m._get_test_data()[:2], 2, 7, m._get_test_data()[2])
    assert np.allclose(s, case['X'][case['test_users'][2:7]] @ case['Y'].T, rtol=0, atol=1e-13)


def test_warm_start_on_the_cpu_double():
    w = ref.warm_case('r5')
    case = w['case']
    m = ref.model_for(case, ref.LMFNumpyOps(), data=ref.warm_data(w))
    m.fold_in_epochs = 4
    m.build()
    assert m.factors['itemid'].tobytes() == case['Y'].tobytes()
    tu, ti, tf = w['test']
    keep = tf != 1.
    assert (~keep).sum() >= w['n_new']
    Cw = sps.csr_matrix((np.log2(tf[keep]), (tu[keep], ti[keep])), shape=(w['n_new'], case['n_items']))
    Cw.sort_indices()
    want = ref.fold_in(Cw, case['Y'], ref.LEARNING_RATE, ref.REGULARIZATION, case['neg_prop'], case['seed'], 4)
    assert m.fold_in().numpy().tobytes() == want.tobytes()
    nothing = np.diff(Cw.indptr) == 0                                    # a user whose known feedback is all 1 keeps the start
    assert not want[nothing][:, :-1].any() and (want[:, -1] == 1).all() and want[~nothing][:, :-1].all()
    recs = m.get_recommendations()
    lists, gaps = ref.lists_and_gaps(want @ case['Y'].T, (tu, ti))
    ref.check_lists(recs, lists, gaps)
    for u in range(w['n_new']):
        assert not set(recs[u]) & set(ti[tu == u])                      # confidence-0 test items are seen items too


def test_scaled_composition_passes_the_scaled_values_to_confidence():
    case = ref.model_case('r5')
    seen = []

    def weight(v):
        seen.append(np.array(v))
        return np.log2(v)
    m = ref.model_for(case, ref.LMFNumpyOps(), cls=ScaledLMF)
    assert m.method == 'LMF-s'
    m.weight_func, m.epsilon, m.num_epochs = weight, 0.25, 1
    m.build()
    scaled = m.get_training_matrix()
    scaled.sort_indices()
    assert len(seen) == 1 and np.allclose(seen[0], scaled.data / 0.25, rtol=1e-15, atol=0)
    plain = ref.model_for(case, ref.LMFNumpyOps())
    plain.epsilon, plain.num_epochs = 0.25, 1
    plain.build()
    assert ref.rel_distance(m.factors['userid'], plain.factors['userid']) > 1e-3
