"""HybridSVD on the device: the dense Cholesky factor (pk_chol_f64) against SciPy, the triangular products and solve
against NumPy, the model against the reference's fixtures (tests/golden/hybrid_*.npz) and the restatement of
tests/hybrid_reference.py, and the scoring pass with separate fold-in factors against brute force."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sps
import torch

import hybrid_reference as ref
from conftest import load_golden
from i2i_reference import tie_aware_mismatches
from test_hybrid_host import FIXTURES, model_for

pytestmark = pytest.mark.gpu


def _spd(n, rng, beta):
    G = rng.standard_normal((n, n)) / np.sqrt(n)
    return G @ G.T + (0.5 if beta == 0 else 0.0) * np.eye(n) + beta * np.eye(n)


@pytest.mark.parametrize('n', [1, 15, 16, 17, 64, 200, 1000, 4099])
@pytest.mark.parametrize('beta', [0.0, 0.7])
def test_cholesky_matches_scipy(n, beta, hip_ops):
    rng = np.random.default_rng(n)
    K = _spd(n, rng, beta)
    img = hip_ops.chol_image(K)
    hip_ops.chol(img, n)
    full = hip_ops.to_host(img)
    L = full[:n, :n]
    assert not np.triu(L, 1).any()
    pad = full.shape[0] - n
    assert np.array_equal(full[n:, n:], np.eye(pad)) and not full[:n, n:].any() and not full[n:, :n].any()
    res = np.linalg.norm(L @ L.T - K) / np.linalg.norm(K)
    assert res <= 4 * n * 2.0 ** -53
    Ls = scipy.linalg.cholesky(K, lower=True)
    assert np.abs(L - Ls).max() <= 1e-10 * np.abs(Ls).max()


def test_densify_in_internal_order(hip_ops):
    rng = np.random.default_rng(3)
    n = 300
    F = sps.random(n, 40, density=0.1, random_state=4, format='csr')
    S = (F @ F.T).tocsr()
    S.setdiag(1.0)
    perm = rng.permutation(n)
    img = hip_ops.hybrid_densify(S, perm, 0.25)
    K = hip_ops.to_host(img)
    expect = np.zeros_like(K)
    Kd = S.toarray() + 0.25 * np.eye(n)
    inv = np.argsort(perm)
    expect[:n, :n] = np.tril(Kd[np.ix_(inv, inv)])
    assert np.array_equal(K, expect)


def test_failing_pivot_names_the_column_and_nothing_sticks(hip_ops):
    n, bad = 300, 137
    K = _spd(n, np.random.default_rng(1), 0.0)
    K[bad, :] = K[:, bad] = 0.0
    K[bad, bad] = -1.0
    img = hip_ops.chol_image(K)
    with pytest.raises(np.linalg.LinAlgError, match='column %d' % bad) as exc:
        hip_ops.chol(img, n)
    assert exc.value.column == bad
    assert np.isfinite(hip_ops.to_host(img)).all()
    Kn = K.copy()
    Kn[bad, bad] = np.nan
    with pytest.raises(np.linalg.LinAlgError, match='column %d' % bad):
        hip_ops.chol(hip_ops.chol_image(Kn), n)
    good = _spd(n, np.random.default_rng(2), 0.3)                    # the next call on the same ops works
    img = hip_ops.chol_image(good)
    hip_ops.chol(img, n)
    assert np.allclose(hip_ops.to_host(img)[:n, :n], np.linalg.cholesky(good), rtol=0, atol=1e-12)


@pytest.mark.parametrize('n', [17, 200, 4099])
@pytest.mark.parametrize('nc', [1, 7, 16, 50, 64, 100])
def test_triangular_products(n, nc, hip_ops):
    rng = np.random.default_rng(n + nc)
    K = _spd(n, rng, 0.2)
    img = hip_ops.chol_image(K)
    hip_ops.chol(img, n)
    L = np.tril(hip_ops.to_host(img)[:n, :n])
    X = rng.standard_normal((n, nc))
    for trans in (False, True):
        Y = hip_ops.to_host(hip_ops.trmm(img, n, hip_ops.to_device(X), trans=trans))
        E = (L.T if trans else L) @ X
        assert np.abs(Y - E).max() <= 1e-12 * np.abs(E).max() * max(1.0, np.sqrt(n) / 8)
    out = torch.zeros(n, 2 * nc, dtype=torch.float64, device=hip_ops.device)
    hip_ops.trmm(img, n, hip_ops.to_device(X), out=out[:, :nc])                # strided destination
    assert np.allclose(hip_ops.to_host(out)[:, :nc], L @ X, rtol=1e-12, atol=1e-12) and not hip_ops.to_host(out)[:, nc:].any()


@pytest.mark.parametrize('n', [17, 200, 4099])
@pytest.mark.parametrize('r', [1, 10, 50, 130])
def test_triangular_solve(n, r, hip_ops):
    rng = np.random.default_rng(7 * n + r)
    K = _spd(n, rng, 0.5)
    img = hip_ops.chol_image(K)
    hip_ops.chol(img, n)
    L = np.tril(hip_ops.to_host(img)[:n, :n])
    B = rng.standard_normal((n, r))
    X = hip_ops.to_host(hip_ops.trsm(img, n, B))
    E = scipy.linalg.solve_triangular(L, B, lower=True, trans='T')
    assert np.abs(X - E).max() <= 1e-12 * np.abs(E).max()


@pytest.mark.parametrize('name', FIXTURES)
def test_model_matches_the_reference(name, hip_ops):
    g = load_golden(name)
    m = model_for(g, hip_ops)
    recs = m.recommendations
    assert m.method == str(g['model'])
    assert np.allclose(m.factors['singular_values'], g['sigma'], rtol=1e-9, atol=0)
    vl, vr = m.get_item_projector()
    assert ref.same_up_to_sign(vl, g['vl'], 1e-8) and ref.same_up_to_sign(vr, g['vr'], 1e-8)
    sigma, _, _, scores, cls, lists = ref.fixture_model(g)
    assert tie_aware_mismatches(recs, g['recs'], scores, cls, tol=1e-9) == []
    test_data, test_shape, _ = m._get_test_data()
    k = g['scores'].shape[0]
    dense, _ = m.slice_recommendations(test_data, test_shape, 0, k)
    assert np.allclose(dense, g['scores'], rtol=1e-9, atol=1e-9 * np.abs(g['scores']).max())
    m.rank = 5
    recs5 = m.recommendations
    assert len(m.training_time) == 1
    s5 = np.asarray(ref.test_matrix(g)[0] @ vr[:, :5]) @ vl[:, :5].T
    cls5 = cls
    assert tie_aware_mismatches(recs5, g['recs_rank5'], s5, cls5, tol=1e-9) == []


def test_features_weight_reproduces_the_other_fixture(hip_ops):
    a, b = load_golden('hybrid_weight_02'), load_golden('hybrid_weight_09')
    m = model_for(a, hip_ops)
    first = m.recommendations
    assert np.array_equal(first, a['recs']) or tie_aware_mismatches(first, a['recs'], *ref.fixture_model(a)[3:5], tol=1e-9) == []
    m.features_weight = 0.9
    assert not m._is_ready
    recs = m.recommendations
    assert np.allclose(m.factors['singular_values'], b['sigma'], rtol=1e-9)
    assert tie_aware_mismatches(recs, b['recs'], *ref.fixture_model(b)[3:5], tol=1e-9) == []
    assert len(m.training_time) == 2


def test_return_factors_and_evaluate(hip_ops):
    g = load_golden('hybrid_known')
    m = model_for(g, hip_ops)
    m.build(return_factors=True)
    n_users = int(g['train_shape'][0])
    assert m.factors['userid'].shape == (n_users, 10)
    W = m.factors['itemid']
    vl, vr = m.get_item_projector()
    F = m.item_cholesky_factor
    assert np.allclose(F.dot(W), vr, atol=1e-10) and np.allclose(F.T.solve(W), vl, atol=1e-9)
    full = m.recommendations
    saved = m.factors                                         # a rank-sweep pipeline swaps `factors` behind the model
    m.rank = 5
    m.recommendations
    m.factors = saved
    m._recommendations = None
    assert np.array_equal(m.recommendations, full)            # the image follows the projector arrays
    assert m._factor_src is saved['itemid_projector_left']


def _brute(T, seen, vl, vr, topk, filter_seen):
    scores = np.asarray(T @ vr) @ vl.T
    cls = np.ones(scores.shape, dtype=np.int64)
    if filter_seen:
        cls[seen] = 0
    items = np.arange(scores.shape[1])
    lists = np.stack([np.lexsort((items, -scores[r], -cls[r]))[:topk] for r in range(scores.shape[0])])
    return scores, cls, lists


@pytest.mark.parametrize('n_users,n_items,rank,topk', [(500, 300, 10, 10), (2000, 1500, 50, 20), (300, 400, 64, 60),
                                                       (200, 350, 300, 10), (9000, 700, 16, 5)])
@pytest.mark.parametrize('filter_seen', [True, False])
def test_recommend_with_fold_in_factors(n_users, n_items, rank, topk, filter_seen, hip_ops):
    from polara_amd import scoring
    rng = np.random.default_rng(n_users + rank + topk)
    vl = rng.standard_normal((n_items, rank)) * rng.uniform(0.2, 2.0, (n_items, 1))
    vr = rng.standard_normal((n_items, rank))
    per = rng.integers(1, 12, n_users)
    rows = np.repeat(np.arange(n_users), per)
    cols = np.concatenate([rng.choice(n_items, k, replace=False) for k in per])
    vals = rng.integers(1, 6, len(rows)).astype(np.float64)
    T = sps.csr_matrix((vals, (rows, cols)), shape=(n_users, n_items))
    T.sort_indices()
    seen = T.toarray() != 0
    D = hip_ops.csr(T.indptr.astype(np.int64), T.indices.astype(np.int32), T.data, T.shape)
    F = scoring.FactorImage(hip_ops, hip_ops.to_device(vl), fold=hip_ops.to_device(vr))
    got = hip_ops.to_host(scoring.recommend(hip_ops, F, D, topk, filter_seen))
    scores, cls, lists = _brute(T, seen, vl, vr, topk, filter_seen)
    assert tie_aware_mismatches(got, lists, scores, cls, tol=1e-12) == []
    ids, sc = scoring.recommend(hip_ops, F, D, topk, filter_seen, return_scores=True)
    ids = hip_ops.to_host(ids)
    assert np.allclose(hip_ops.to_host(sc), np.take_along_axis(scores, ids, 1), rtol=1e-12, atol=1e-12)
    dense = hip_ops.to_host(scoring.dense_scores(hip_ops, F, D, 0, min(50, n_users)))
    assert np.allclose(dense, scores[:min(50, n_users)], rtol=1e-12, atol=1e-12)


def test_ml1m_shaped_against_the_restatement(hip_ops):
    from polara_amd import synth
    from polara_amd.data import SimilarityArrayData
    from polara_amd.models import HybridSVD
    csr, _ = synth.make_workload('ml1m')
    rows, cols, vals = synth.csr_to_coo_triplets(csr)
    shp = tuple(int(x) for x in csr['shape'])
    n_users, n_items = shp
    rng = np.random.default_rng(5)
    Fm = sps.csr_matrix((rng.random((n_items, 200)) < 0.03).astype(np.float64))
    Fm = Fm + sps.csr_matrix((np.ones(n_items), (np.arange(n_items), rng.integers(0, 200, n_items))), shape=Fm.shape)
    Fm.data[:] = 1.0
    nrm = np.sqrt(np.asarray(Fm.multiply(Fm).sum(1)).ravel())
    Fn = sps.diags(1 / nrm) @ Fm
    S = (Fn @ Fn.T).tocsr()
    S.setdiag(1.0)
    d = SimilarityArrayData((rows, cols, vals), n_users=n_users, n_items=n_items,
                            relations_matrices={'itemid': S}, relations_indices={'itemid': None})
    m = HybridSVD(d, ops=hip_ops)
    m.verbose = False
    m.rank = 20
    m.build()
    A = sps.csr_matrix((vals, (rows, cols)), shape=shp)
    L = ref.cholesky_factor(S, 0.5)
    sigma = np.linalg.svd(np.asarray(A @ L), compute_uv=False)[:20]
    assert np.allclose(m.factors['singular_values'], sigma, rtol=1e-9)
