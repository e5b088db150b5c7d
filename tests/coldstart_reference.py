"""Item cold start restated in NumPy / SciPy (coldstart/models.py:149-257): the parent's factors (PureSVD: SVD of A;
HybridSVD: tests/hybrid_reference.py), W = F_train^T P with P = V or vr, G = pinv(W^T W), scores (F_cold W) G (U diag(sigma))^T
and the lists (ties to the lower user index).  Used by the host tests against the reference's fixtures and by the device
tests and the benchmark as the CPU side."""
import numpy as np
import scipy.sparse as sps

import hybrid_reference as href


def one_hot(g, which):
    shape = tuple(int(x) for x in g[which + '_shape'])
    r, c = g[which + '_row'], g[which + '_col']
    return sps.csr_matrix((np.ones(len(r)), (r, c)), shape=shape)


def svd_factors(A, rank):
    u, s, vt = np.linalg.svd(A.toarray() if sps.issparse(A) else A, full_matrices=False)
    return u[:, :rank], s[:rank], vt[:rank].T


def embeddings(F_train, P):
    """(W, G)"""
    W = np.asarray(F_train.T @ P)
    return W, np.linalg.pinv(W.T @ W)


def scores(F_cold, W, G, U, sigma):
    return (np.asarray(F_cold @ W) @ G) @ (U * sigma[None, :]).T


def lists(s, topk):
    users = np.arange(s.shape[1])
    out = np.empty((s.shape[0], topk), dtype=np.int64)
    for r in range(s.shape[0]):
        out[r] = np.lexsort((users, -s[r]))[:topk]
    return out


def truncated(W, U, sigma, rank):
    """the reference's rank reduction (coldstart/models.py:169-183): leading columns, G recomputed"""
    W5 = W[:, :rank]
    return W5, np.linalg.pinv(W5.T @ W5), U[:, :rank], sigma[:rank]


def fixture_model(g):
    """The restatement on a fixture: dict(sigma, U, P, W, G, scores, lists, lists5)."""
    name = str(g['model'])
    scaled = name.endswith('-s')
    rank, topk = int(g['rank']), int(g['topk'])
    A = href.training_matrix(g, scaled=scaled)
    if name.startswith('HybridSVD'):
        L = href.cholesky_factor(href.relations(g), float(g['features_weight']))
        M = np.asarray(A @ L)
        u, s, vt = np.linalg.svd(M, full_matrices=False)
        U, sigma = u[:, :rank], s[:rank]
        P = L @ vt[:rank].T                      # the right projector
    else:
        U, sigma, P = svd_factors(A, rank)
    Ft, Fc = one_hot(g, 'ft'), one_hot(g, 'fc')
    W, G = embeddings(Ft, P)
    s = scores(Fc, W, G, U, sigma)
    W5, G5, U5, s5 = truncated(W, U, sigma, 5)
    return dict(sigma=sigma, U=U, P=P, W=W, G=G, scores=s, lists=lists(s, topk),
                lists5=lists(scores(Fc, W5, G5, U5, s5), topk), G5=G5)


def queries(indptr, indices, values, W, G):
    """E = (F W) G row by row, the labels of a row in their stored order: what `HipOps.coldstart_queries` computes"""
    n = len(indptr) - 1
    F = sps.csr_matrix((np.ones(len(indices)) if values is None else values, indices, indptr), shape=(n, W.shape[0]))
    return np.asarray(F @ W) @ G


same_up_to_sign = href.same_up_to_sign
