"""EASE on the device: the in-place triangular inverse (pk_trtri_f64) against SciPy's substitution, the Gram diagonal, the
weights image (pk_ease_weights_f64) against the restatement of tests/ease_reference.py and against np.linalg.inv's own
residual, determinism, the failure path of a singular Gram matrix, and the model: lists, scores, slices, lifecycle, limits.

Every bound compares with what the reference routine achieves on the same input (printed next to the device's figure:
run with -s to see the ratios DESIGN.md 8l quotes)."""
import numpy as np
import pytest
import scipy.linalg

import ease_reference as ref
import i2i_reference as i2i_ref
from item_model_helpers import cached_fixture, device_csr as _device_csr, limits_case, model
from test_gpu_hybrid import _spd

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 63, 64, 65, 129, 200, 1000, 4099]      # around the 16-wide MFMA tile and the 64-wide block


# ---- triangular inverse ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('beta', [0.0, 0.7])
def test_triangular_inverse_against_scipy(n, beta, hip_ops):
    K = _spd(n, np.random.default_rng(n), beta)
    img = hip_ops.chol_image(K)
    hip_ops.chol(img, n)
    L = hip_ops.to_host(img)[:n, :n].copy()
    hip_ops.trtri(img, n)
    full = hip_ops.to_host(img)
    W = full[:n, :n]
    assert not np.triu(W, 1).any()
    pad = full.shape[0] - n
    assert np.array_equal(full[n:, n:], np.eye(pad)) and not full[:n, n:].any() and not full[n:, :n].any()
    eye = np.eye(n)
    r = np.abs(W @ L - eye).max()
    r_ref = np.abs(scipy.linalg.solve_triangular(L, eye, lower=True) @ L - eye).max()
    print('trtri n=%d beta=%.1f: max|WL - I| = %.3e, solve_triangular %.3e, ratio %.2f' % (n, beta, r, r_ref, r / r_ref if r_ref else 0))
    # 4 x: a blocked MFMA summation order is not LAPACK's; both are backward-stable substitutions of one bound class
    assert r <= 4 * r_ref


# ---- weights -----------------------------------------------------------------------------------------------------------
def _device_weights(hip_ops, idx, val, shape, lam, implicit=False):
    """(B image, d) on the host through the four stages of the build."""
    n = shape[1]
    img = hip_ops.ease_gram(_device_csr(hip_ops, idx, val, shape, implicit), lam)
    hip_ops.chol(img, n)
    hip_ops.trtri(img, n)
    B, d = hip_ops.ease_weights(img, n)
    return hip_ops.to_host(B), hip_ops.to_host(d)


def _check_weights(tag, Bimg, d, A, lam, floor=0.0):
    """The checks of a weights image against the restatement on the SciPy matrix A: pad columns and diagonal exactly 0,
    max|P K - I| of the P rebuilt from (B, d) within 4 x the same residual of np.linalg.inv (`floor`: see
    test_weights_at_the_tile_edges), max|B - B_ref| <= 1e-12 max|B_ref|."""
    from polara_amd import i2i
    n = A.shape[1]
    assert Bimg.shape == (n, i2i.leading_dim(n)) and d.shape == (n,)
    assert not Bimg[:, n:].any()                                           # pad columns exactly 0
    B = Bimg[:, :n]
    assert not np.diag(B).any() and np.isfinite(B).all() and (d > 0).all()
    B_ref, P_ref = ref.ease_weights(A, lam)
    K = ref.gram(A, lam)
    r = ref.inverse_residual(ref.precision_from_weights(B, d), K)
    r_ref = ref.inverse_residual(P_ref, K)
    dist = np.abs(B - B_ref).max()
    scale = np.abs(B_ref).max()
    print('%s: max|P K - I| = %.3e, np.linalg.inv %.3e, ratio %.2f; max|B - B_ref| = %.2e of max|B_ref| = %.3g'
          % (tag, r, r_ref, r / r_ref if r_ref else 0, dist, scale))
    assert r <= 4 * max(r_ref, floor)
    assert dist <= 1e-12 * scale


def _sized_training(n):
    """Seeded integer-valued X with n items: 3 n users (at least 8) of up to 10 items each, every item present."""
    rng = np.random.default_rng(5000 + n)
    n_users, per = max(8, 3 * n), min(n, 10)
    us, its = [], []
    for u in range(n_users):
        k = int(rng.integers(1, per + 1))
        its.append(rng.choice(n, k, replace=False))
        us.append(np.full(k, u))
    us, its = np.concatenate(us), np.concatenate(its)
    missing = np.setdiff1d(np.arange(n), its)
    pairs = np.unique(np.stack([np.r_[us, rng.integers(0, n_users, len(missing))], np.r_[its, missing]], 1), axis=0)
    return pairs.astype(np.int64), rng.integers(1, 6, len(pairs)).astype(np.float64), (n_users, n)


@pytest.mark.parametrize('n', SIZES)
def test_weights_at_the_tile_edges(n, hip_ops):
    """The checks of the fixtures at every size around the tiles.  One figure differs: the reference residual gets a floor
    of one unit of fp64 (2^-52).  At n = 1, np.linalg.inv returns fl(1 / K) and fl(fl(1 / K) K) is exactly 1 for most K, so
    4 x that residual is 0 and names no scale, while the Cholesky route takes three roundings (root, quotient, square) and
    cannot be exact; measured there: 3.3e-16 against 0.  From n = 15 on the floor is below every measured reference
    residual (4.7e-16 .. 2.4e-15) and changes nothing."""
    idx, val, shape = _sized_training(n)
    Bimg, d = _device_weights(hip_ops, idx, val, shape, 10.0)
    _check_weights('weights n=%d' % n, Bimg, d, ref.training_matrix(idx, val, shape), 10.0, floor=2.0 ** -52)


_fixture = cached_fixture(ref)


@pytest.mark.parametrize('name', sorted(ref.FIXTURES))
@pytest.mark.parametrize('implicit', [False, True])
@pytest.mark.parametrize('lam', ref.LAMBDAS)
def test_weights_and_residual_on_the_fixtures(name, implicit, lam, hip_ops):
    idx, val, shape, A = _fixture(name, implicit)
    Bimg, d = _device_weights(hip_ops, idx, val, shape, lam, implicit)
    _check_weights('weights %s implicit=%d lam=%g' % (name, implicit, lam), Bimg, d, A, lam)


@pytest.mark.parametrize('name', sorted(ref.FIXTURES))
@pytest.mark.parametrize('half_steps', [False, True])
def test_gram_image_is_exact(name, half_steps, hip_ops):
    from polara_amd import ease
    idx, val, shape = ref.training(name, half_steps)
    n, lam = shape[1], 0.5
    X = ref.training_matrix(idx, val, shape)
    img = hip_ops.to_host(hip_ops.ease_gram(_device_csr(hip_ops, idx, val, shape), lam))
    assert img.shape == (ease.chol_leading_dim(n),) * 2
    want = np.asarray(X.multiply(X).sum(0)).ravel() + lam
    assert np.array_equal(np.diag(img)[:n], want)
    G = np.asarray((X.T @ X).todense())
    assert np.array_equal(np.tril(img[:n, :n], -1), np.tril(G, -1))         # what the factorisation reads


# ---- determinism and the failure path -----------------------------------------------------------------------------------
def _model(hip_ops, idx, val, shape, test=None, holdout=None, lam=10.0, implicit=False):
    return model('EASEModel', hip_ops, idx, val, shape, test, holdout, regularization=lam, implicit=implicit)


def test_two_builds_give_the_same_bits(hip_ops):
    idx, val, shape = ref.training('large')
    m = _model(hip_ops, idx, val, shape)
    m.build()
    B1, d1 = hip_ops.to_host(m.item_weights).copy(), m.precision_diagonal.copy()
    m.build()
    assert np.array_equal(B1, hip_ops.to_host(m.item_weights)) and np.array_equal(d1, m.precision_diagonal)
    assert len(m.training_time) == 2
    assert {'n_items', 'nnz', 'image_bytes', 'gram_s', 'chol_s', 'trtri_s', 'weights_s'} <= set(m.build_stats)


def test_singular_gram_names_the_item_and_nothing_sticks(hip_ops):
    idx, val, shape = ref.training('small')
    empty = 57
    keep = idx[:, 1] != empty
    idx, val = idx[keep], val[keep]
    m = _model(hip_ops, idx, val, shape, lam=0.0)
    with pytest.raises(np.linalg.LinAlgError, match='column %d' % empty) as exc:
        m.build()
    assert exc.value.column == empty
    assert m.item_weights is None and m.precision_diagonal is None and not m._is_ready
    m.regularization = 1.0                                      # the next build on the same ops works
    m.build()
    Bimg = hip_ops.to_host(m.item_weights)
    _check_weights('after the failure', Bimg, m.precision_diagonal, ref.training_matrix(idx, val, shape), 1.0)


# ---- model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(ref.FIXTURES))
@pytest.mark.parametrize('implicit', [False, True])
def test_model_lists_and_scores_match_the_restatement(name, implicit, hip_ops):
    idx, val, shape, A = _fixture(name, implicit)
    test, holdout, tshape = ref.test_rows(name)
    lam = 10.0
    m = _model(hip_ops, idx, val, shape, test, holdout, lam, implicit)
    m.build()
    B_ref, _ = ref.ease_weights(A, lam)
    T, seen = i2i_ref.test_matrix(test, tshape, implicit)
    scores = ref.ease_scores(B_ref, T)
    assert not scores[-1].any() and not scores[1].any() and seen[1].any()       # an empty row and a zero-feedback row
    for filter_seen in (True, False):
        cls = i2i_ref.classes(scores, seen, filter_seen, False)
        for topk in (1, 10, 100):
            m.filter_seen, m.topk = filter_seen, topk
            recs = m.get_recommendations()
            want = i2i_ref.select(scores, seen, topk, filter_seen, False)
            assert recs.shape == want.shape and recs.dtype == np.int64 and (recs >= 0).all()
            assert i2i_ref.tie_aware_mismatches(recs, want, scores, cls, tol=1e-9) == [], (filter_seen, topk)
            lists, list_scores = m.recommend_with_scores()
            assert np.array_equal(lists, recs)
            s_ref = np.take_along_axis(scores, lists, 1)
            assert (np.abs(list_scores - s_ref) <= 1e-9 * np.maximum(1, np.abs(s_ref))).all()
    assert len(m.training_time) == 1
    test_data, test_shape, _ = m._get_test_data()
    block, triplet = m.slice_recommendations(test_data, test_shape, 3, 17)
    assert isinstance(block, np.ndarray) and block.shape == (14, shape[1])
    assert (np.abs(block - scores[3:17]) <= 1e-9 * np.maximum(1, np.abs(scores[3:17]))).all()
    assert np.array_equal(triplet[1], test[1][(test[0] >= 3) & (test[0] < 17)])


def test_lifecycle(hip_ops):
    idx, val, shape = ref.training('medium')
    test, holdout, tshape = ref.test_rows('medium')
    m = _model(hip_ops, idx, val, shape, test, holdout, lam=500.0)
    m.topk = 10
    recs = m.recommendations
    assert recs.shape == (tshape[0], 10) and len(m.training_time) == 1
    m.regularization = 500                                      # unchanged: the model and its lists stay
    assert m.recommendations is recs and m._is_ready and len(m.training_time) == 1
    m.topk = 20                                                 # growing re-scores, no rebuild
    assert np.array_equal(m.recommendations[:, :10], recs) and len(m.training_time) == 1
    m.regularization = 5.0                                      # a change: the image is dropped at once, then rebuilt
    assert m.item_weights is None and not m._is_ready
    other = m.recommendations
    assert len(m.training_time) == 2 and m.item_weights is not None
    B_ref, _ = ref.ease_weights(ref.training_matrix(idx, val, shape), 5.0)
    T, seen = i2i_ref.test_matrix(test, tshape)
    scores = ref.ease_scores(B_ref, T)
    want = i2i_ref.select(scores, seen, 20, True, False)
    assert i2i_ref.tie_aware_mismatches(other, want, scores, i2i_ref.classes(scores, seen, True, False), tol=1e-9) == []
    top, seen_items = m.show_recommendations(5, topk=10)
    assert np.array_equal(top, other[5, :10]) and set(seen_items) == set(test[1][test[0] == 5])
    assert m.evaluate(topk=10) is not None
    m.data.set_training_data((idx[:, 0], idx[:, 1], val * 2))    # a data change: a new model
    assert m.item_weights is None and not m._is_ready


def test_stated_limits(hip_ops, monkeypatch):
    from polara_amd import ease
    pairs, val, (n_users, n_items), hold = limits_case()
    m = _model(hip_ops, pairs, val, (n_users, n_items), holdout=hold, lam=1.0)
    m.topk = 1024
    assert m.recommendations.shape == (n_users, 1024)
    m.topk = 1025
    with pytest.raises(ValueError, match='1024'):
        m.get_recommendations()
    with pytest.raises(ValueError, match='1024'):
        m.recommend_with_scores()
    # the guard speaks before anything is allocated: a fake free-bytes figure, not an exhausted device
    need = ease.chol_image_bytes(n_items) + ease.weights_image_bytes(n_items)
    monkeypatch.setattr(hip_ops, 'free_bytes', lambda: 2 * need - 16)
    with pytest.raises(MemoryError, match=str(need)):
        m.build()
    assert m.item_weights is None
    monkeypatch.setattr(hip_ops, 'free_bytes', lambda: 2 * need)
    m.build()
    assert m.item_weights is not None
