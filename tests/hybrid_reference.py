"""HybridSVD restated in NumPy / SciPy (hybrid/models.py:228-397): K = S + beta I, a dense lower Cholesky factor L, the SVD
of A L, the projectors vl = L^-T W and vr = L W, scores T vr vl^T and the lists (seen items last under filter_seen,
ties to the lower item index).  Used by the host tests against the reference's fixtures and by the device tests."""
import numpy as np
import scipy.linalg
import scipy.sparse as sps

from polara_amd.hybrid import beta_of


def relations(g):
    n = int(g['train_shape'][1])
    return sps.csr_matrix((g['rel_val'], (g['rel_row'], g['rel_col'])), shape=(n, n))


def training_matrix(g, scaled=False, col_scaling=0.4, row_scaling=1.0):
    idx = g['train_idx']
    shp = tuple(int(x) for x in g['train_shape'])
    A = sps.csr_matrix((g['train_val'], (idx[:, 0], idx[:, 1])), shape=shp, dtype=np.float64)
    if scaled:                          # ScaledMatrixMixin (models.py:864-895): D_r A D_c, D = sqrt(nnz)^(scaling - 1)
        rn = np.diff(A.indptr).astype(np.float64)
        cn = np.bincount(A.indices, minlength=shp[1]).astype(np.float64)
        rs, cs = np.ones_like(rn), np.ones_like(cn)
        np.power(np.sqrt(rn), row_scaling - 1, where=rn != 0, out=rs)
        np.power(np.sqrt(cn), col_scaling - 1, where=cn != 0, out=cs)
        A = sps.diags(rs) @ A @ sps.diags(cs)
    return A.tocsr()


def cholesky_factor(S, weight):
    K = (S.toarray() if sps.issparse(S) else np.asarray(S, dtype=np.float64)) + beta_of(weight) * np.eye(S.shape[0])
    return np.linalg.cholesky(K)


def build(A, L, rank):
    """(sigma, W, vl, vr) of the SVD of A L."""
    M = (A @ L) if not sps.issparse(A) else np.asarray(A @ L)
    _, s, vt = np.linalg.svd(M, full_matrices=False)
    W = vt[:rank].T
    vl = scipy.linalg.solve_triangular(L, W, lower=True, trans='T')
    vr = L @ W
    return s[:rank], W, vl, vr


def test_matrix(g, n_users=None):
    shape = tuple(int(x) for x in g['test_shape'])[:2]
    u, i, f = g['test_user'], g['test_item'], g['test_fdbk']
    keep = f != 0
    T = sps.csr_matrix((f[keep], (u[keep], i[keep])), shape=shape)
    seen = np.zeros(shape, dtype=bool)
    seen[u, i] = True
    return T, seen


def scores_and_lists(T, seen, vl, vr, topk, filter_seen=True):
    """(scores [n_users x n_items], class (1 = candidate, 0 = seen under filter_seen), lists)."""
    scores = np.asarray(T @ vr) @ vl.T
    cls = np.ones(scores.shape, dtype=np.int64)
    if filter_seen:
        cls[seen] = 0
    items = np.arange(scores.shape[1])
    lists = np.empty((scores.shape[0], topk), dtype=np.int64)
    for r in range(scores.shape[0]):
        order = np.lexsort((items, -scores[r], -cls[r]))
        lists[r] = order[:topk]
    return scores, cls, lists


def fixture_model(g):
    """The restatement on a fixture: (sigma, vl, vr, scores, class, lists)."""
    scaled = str(g['model']).endswith('-s')
    A = training_matrix(g, scaled=scaled)
    L = cholesky_factor(relations(g), float(g['features_weight']))
    sigma, _, vl, vr = build(A, L, int(g['rank']))
    T, seen = test_matrix(g)
    scores, cls, lists = scores_and_lists(T, seen, vl, vr, int(g['topk']), bool(g['filter_seen']))
    return sigma, vl, vr, scores, cls, lists


def same_up_to_sign(a, b, tol):
    """max deviation of the columns of a from those of b with the signs aligned, relative to max |b|."""
    s = np.sign(np.sum(a * b, axis=0))
    s[s == 0] = 1
    return float(np.abs(a - b * s).max() / max(1e-300, np.abs(b).max())) <= tol
