"""SLIM, host side (no GPU): the two NumPy restatements of the solver's contract against each other (tests/slim_reference.py:
the plain loop and the screened form the kernel is modelled on), the restatement against scikit-learn's ElasticNet, the
planning and the guards of the device path (polara_amd/slim.py) against the library's pk_slim_* planning functions, the
parameter checks and the export."""
import numpy as np
import pytest

import slim_reference as ref


def _gram(name, implicit=False):
    idx, val, shape = ref.training(name)
    return ref.gram(ref.training_matrix(idx, val, shape, implicit))


@pytest.mark.parametrize('name,step,positive', [('small', 1, True), ('medium', 16, True), ('small', 8, False),
                                                ('medium', 64, False)])
def test_screened_form_equals_the_plain_loop(name, step, positive):
    """Bits and sweep counts: `small` on all columns, `medium` on every 16th; without the sign constraint (dense
    solutions: every coordinate changes in every sweep, the plain loop's slowest case) on fewer columns."""
    G = _gram(name)
    cols = range(0, G.shape[0], step)
    for l1, l2 in ((1.0, 5.0), (5.0, 0.5)) if positive else ((3.0, 20.0),):
        Wp, sp = ref.solve_columns(G, cols, l1, l2, plain=True, positive=positive)
        Ws, ss = ref.solve_columns(G, cols, l1, l2, positive=positive)
        assert np.array_equal(Wp, Ws) and np.array_equal(sp, ss)
        assert np.count_nonzero(Wp) > 0 and sp.max() > 1
        assert not positive or sp.max() <= 38                            # with the sign constraint the cap of 100 does not bind
        assert not Wp[np.arange(len(cols)), list(cols)].any()
        assert positive == bool((Wp >= 0).all())


def test_cap_and_degenerate_columns():
    G = _gram('small')
    Wp, sp = ref.solve_columns(G, range(0, 120, 7), 1.0, 5.0, max_sweeps=3, plain=True)
    Ws, ss = ref.solve_columns(G, range(0, 120, 7), 1.0, 5.0, max_sweeps=3)
    assert np.array_equal(Wp, Ws) and np.array_equal(sp, ss) and (sp == 3).any() and sp.max() == 3
    # an item without training entries and l2 = 0: den = 0, the coordinate is skipped; as a target its column is empty
    G0 = G.copy()
    G0[57, :] = 0
    G0[:, 57] = 0
    for solve in (ref.solve_column_plain, ref.solve_column):
        w, s = solve(G0, 57, 1.0, 0.0, 1e-4, 100)
        assert not w.any() and s == 1
        w, s = solve(G0, 3, 1.0, 0.0, 1e-4, 100)
        assert w[57] == 0 and np.isfinite(w).all() and w.any()


@pytest.mark.parametrize('l1,l2', [(1.0, 5.0), (5.0, 0.5), (20.0, 50.0)])
def test_restatement_reaches_sklearn_optimum(l1, l2):
    """ElasticNet minimises 1 / (2 m) |y - X w|^2 + alpha rho |w|_1 + alpha (1 - rho) / 2 |w|^2: alpha rho m = l1 and
    alpha (1 - rho) m = l2.  Both run to tol 1e-10; the restatement's objective may exceed sklearn's by 1e-12 relative."""
    linear_model = pytest.importorskip('sklearn.linear_model')
    idx, val, shape = ref.training('small')
    X = np.asarray(ref.training_matrix(idx, val, shape).todense())
    G = ref.gram(ref.training_matrix(idx, val, shape))
    m = shape[0]
    alpha, rho = (l1 + l2) / m, l1 / (l1 + l2)
    for j in (0, 7, 57, 119):
        w, sweeps = ref.solve_column_plain(G, j, l1, l2, 1e-10, 10000)
        assert sweeps < 10000
        Xj = X.copy()
        Xj[:, j] = 0                                          # the constraint w[j] = 0
        en = linear_model.ElasticNet(alpha=alpha, l1_ratio=rho, positive=True, fit_intercept=False, tol=1e-10, max_iter=100000)
        en.fit(Xj, X[:, j])
        w_sk = np.asarray(en.coef_, dtype=np.float64).copy()
        w_sk[j] = 0
        f, f_sk = ref.objective(X, j, w, l1, l2), ref.objective(X, j, w_sk, l1, l2)
        print('l1=%g l2=%g j=%d: objective %.17g, sklearn %.17g, excess %.2e, max|w - w_sk| = %.2e'
              % (l1, l2, j, f, f_sk, (f - f_sk) / f_sk, np.abs(w - w_sk).max()))
        assert f <= f_sk * (1 + 1e-12)


def test_planning_matches_the_library():
    from polara_amd import _lib, simagg, slim
    lib = _lib.load()
    assert slim.MAX_ITEMS == lib.pk_slim_max_items() >= 26744
    assert slim.LDS_ITEMS == lib.pk_slim_lds_items() and slim.LDS_ITEMS * 8 < 160 * 1024
    assert slim.MAX_TOPK == simagg.MAX_TOPK == lib.pk_i2i_max_topk()
    for n in (1, 2, 7, 8, 9, 63, 64, 65, 257, 1023, 1024, 1025, 2050, 19456, 19457, 26744, 65536):
        assert slim.gram_leading_dim(n) == lib.pk_i2i_ld(n)
        assert slim.gram_image_bytes(n) == n * lib.pk_i2i_ld(n) * 8
        assert slim.default_batch_columns(n) == lib.pk_slim_batch_columns(n) == min(n, 1024)
        assert slim.residual_in_lds(n) == (n <= 19456)
        for nc in (0, 1, 7, min(n, 1024)):
            assert slim.work_bytes(n, nc) == lib.pk_slim_work_bytes(n, nc)
    assert slim.work_bytes(100, 10) == 1024 and slim.work_bytes(100, 10, r_global=True) == 1024 + 10 * 100 * 8
    assert slim.work_bytes(26744, 1024) == 214016 + 1024 * 26744 * 8


def test_the_option_moves_the_residual_rows(pk_options):
    from polara_amd import _lib, slim
    lib = _lib.load()
    assert lib.pk_slim_work_bytes(100, 10) == slim.work_bytes(100, 10, r_global=False)
    pk_options('slim_r_global', 1)
    assert lib.pk_slim_work_bytes(100, 10) == slim.work_bytes(100, 10, r_global=True)


def test_batch_rule_and_memory_guard():
    from polara_amd import slim
    n = 26744
    assert slim.default_batch_columns(n, 200e9) == 1024
    small = slim.default_batch_columns(n, 16 * slim.batch_bytes(n, 100))
    assert 50 <= small <= 100 and slim.batch_bytes(n, small) <= slim.batch_bytes(n, 100)
    assert slim.default_batch_columns(n, 0) == 1 and slim.default_batch_columns(1, 1e9) == 1
    need = slim.gram_image_bytes(n) + slim.batch_bytes(n, 7)
    assert slim.check_build_memory(n, 2 * need, 7) == need
    with pytest.raises(MemoryError, match=str(need)):
        slim.check_build_memory(n, 2 * need - 16, 7)
    with pytest.raises(MemoryError, match=r'5\.7\d GB'):
        slim.check_build_memory(n, 1e9)
    # the dense output never rivals the Gram image
    assert slim.batch_bytes(n, 1024) < slim.gram_image_bytes(n) / 10
    # more items than the solver takes: ValueError naming the limit, whatever the memory
    assert slim.check_items(65536) == 65536
    with pytest.raises(ValueError, match='65536'):
        slim.check_build_memory(65537, 1e15)
    with pytest.raises(ValueError, match='65536'):
        slim.check_items(65537)


def _tiny_data():
    from polara_amd.data import ArrayData
    u, i, v = np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([1.0, 2.0, 3.0])
    return ArrayData((u, i, v), n_users=2, n_items=2)


def test_model_attributes_and_export():
    import polara_amd
    from polara_amd.models import RecommenderModel
    from polara_amd.slim import SLIMModel
    assert polara_amd.SLIMModel is SLIMModel and 'SLIMModel' in polara_amd.__all__
    assert issubclass(SLIMModel, RecommenderModel)
    m = SLIMModel(_tiny_data())
    assert (m.method, m.l1_regularization, m.l2_regularization, m.tolerance, m.max_sweeps) == ('SLIM', 1.0, 10.0, 1e-4, 100)
    assert (m.positive, m.implicit, m.column_batch, m.dense_output, m._topk_limit) == (True, False, None, True, 1024)
    assert m._item_rank is None and m.item_weights is None and m.sweeps is None


def test_bad_parameters_raise():
    from polara_amd import slim
    m = slim.SLIMModel(_tiny_data())
    for name in ('l1_regularization', 'l2_regularization'):
        for bad in (-1.0, -1e-300, float('nan'), float('inf')):
            with pytest.raises(ValueError, match=name):
                setattr(m, name, bad)
        setattr(m, name, 0)                                    # allowed
        assert getattr(m, name) == 0.0
    for bad in (0.0, -1e-4, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='tolerance'):
            m.tolerance = bad
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='max_sweeps'):
            m.max_sweeps = bad
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='column_batch'):
            m.column_batch = bad
    assert (m.tolerance, m.max_sweeps, m.column_batch) == (1e-4, 100, None)
    assert slim.check_parameters(0, 0.5, 1e-10, 7) == (0.0, 0.5, 1e-10, 7)


def test_settings_renew_or_refresh_the_model():
    from polara_amd.slim import SLIMModel
    m = SLIMModel(_tiny_data())

    def arm():
        m._is_ready, m._W, m._recommendations = True, object(), object()
    arm()
    m.l1_regularization, m.l2_regularization, m.tolerance, m.max_sweeps = 1.0, 10, 1e-4, 100    # unchanged: nothing happens
    m.positive, m.implicit, m.column_batch, m.dense_output = True, False, None, True
    assert m._is_ready and m._W is not None and m._recommendations is not None
    for name, value in (('l1_regularization', 2.0), ('l2_regularization', 0.5), ('tolerance', 1e-6), ('max_sweeps', 5),
                        ('positive', False), ('implicit', True), ('column_batch', 7)):
        arm()
        setattr(m, name, value)
        assert not m._is_ready and m._W is None and m._recommendations is None, name
    arm()
    m.dense_output = False                                     # new lists, the same model
    assert m._is_ready and m._W is not None and m._recommendations is None


def test_multi_process_raises():
    from polara_amd.slim import SLIMModel

    class TwoRanks:
        world, rank = 2, 0
    with pytest.raises(NotImplementedError):
        SLIMModel(_tiny_data(), comm=TwoRanks()).build()


def test_topk_above_the_limit_raises():
    from polara_amd import i2i, slim
    assert i2i.check_topk(1024, 5000, slim.SLIMModel._topk_limit) == 1024
    with pytest.raises(ValueError, match='1024'):
        i2i.check_topk(1025, 5000, slim.SLIMModel._topk_limit)
