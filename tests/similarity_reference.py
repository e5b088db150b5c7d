"""Host restatement of the item similarities of polara_amd/similarity.py in SciPy and NumPy: what the device path has to
reproduce bit for bit.  The products are SciPy's own; the weighted Jaccard index walks the pairs that share a label in plain
Python floats (IEEE doubles added one at a time, in the order the contract fixes).  Also the readers of the
tests/golden/similarity_*.npz fixtures."""
import warnings

import numpy as np
import scipy.sparse as sps

KINDS = ('cosine', 'cosine-binary', 'tfidf-cosine', 'jaccard')       # the kinds of the `wide` and `cross` fixtures


def canonical(S):
    S = sps.csr_matrix(S)
    S.sort_indices()
    return S


def same_bits(A, B):
    """Two canonical CSR matrices hold the same pattern and the same bit patterns."""
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(np.asarray(A.data, np.float64).view(np.uint64), np.asarray(B.data, np.float64).view(np.uint64)))


def features(g, prefix='f'):
    """The feature matrix of a fixture as the CSR it was generated from (stored order, explicit zeros kept)."""
    shape = tuple(int(x) for x in g[prefix + '_shape'])
    return sps.csr_matrix((g[prefix + '_data'], g[prefix + '_indices'], g[prefix + '_indptr']), shape=shape)


def stored(g, key):
    """The matrix stored under `key` (indptr, indices, data, shape)."""
    shape = tuple(int(x) for x in g[key + '_shape'])
    return sps.csr_matrix((g[key + '_data'], g[key + '_indices'], g[key + '_indptr']), shape=shape)


def _set_diagonal(S, v):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', category=sps.SparseEfficiencyWarning)
        S.setdiag(v)


def inverse_root(d):
    out = np.zeros(len(d), dtype=np.float64)
    np.power(d, -0.5, where=d > 0, out=out)
    return out


def normalized(F, binary=False):
    F = F.tocsr()
    sq = F.getnnz(axis=1) if binary else np.asarray(F.power(2).sum(axis=1)).reshape(-1)
    return sps.diags(inverse_root(sq)).dot(F)


def tfidf(F, idf_from=None):
    F = F.tocsr()
    G = F if idf_from is None else idf_from
    idf = np.log((1 + G.shape[0]) / (1 + G.getnnz(axis=0)))
    return sps.csr_matrix((np.take(idf, F.indices), F.indices, F.indptr), shape=F.shape)


def cosine(F, fill_diagonal=True, assume_binary=False):
    Fn = normalized(F, assume_binary)
    S = Fn.dot(Fn.T)
    if fill_diagonal:
        _set_diagonal(S, 1)
    return canonical(S)


def _jaccard_divide(S, nf_rows, nf_cols):
    S = sps.csr_matrix(S)
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    S.data = S.data / ((nf_rows[rows] + nf_cols[S.indices]) - S.data)
    return S


def jaccard(F, fill_diagonal=True, counted=True):
    """counted: the intersection counted in fp64 (the contract); else the boolean product as the installed SciPy runs it."""
    P = F.tocsr() != 0
    nf = P.getnnz(axis=1)
    S = P.astype(np.float64).dot(P.T) if counted else P.dot(P.T).astype(np.float64)
    S = _jaccard_divide(S, nf, nf)
    if fill_diagonal:
        _set_diagonal(S, 1)
    return canonical(S)


def _rows(F):
    F = sps.csr_matrix(F, dtype=np.float64, copy=True)
    F.sort_indices()
    return F, [(F.indices[a:b].tolist(), F.data[a:b].tolist()) for a, b in zip(F.indptr[:-1], F.indptr[1:])]


def weighted_pair(row_i, row_j):
    """(min_sum, max_sum) of the pair: over the labels of j ascending a shared label adds min / max, another one dat_j to
    max_sum; then the labels of i alone, ascending."""
    (ci, di), (cj, dj) = row_i, row_j
    at = dict(zip(ci, di))
    in_j = set(cj)
    mn, mx = 0.0, 0.0
    for c, d in zip(cj, dj):
        if c in at:
            mn += min(at[c], d)
            mx += max(at[c], d)
        else:
            mx += d
    for c, d in zip(ci, di):
        if c not in in_j:
            mx += d
    return mn, mx


def jaccard_weighted(F, fill_diagonal=True):
    F, rows = _rows(F)
    n = F.shape[0]
    P = sps.csr_matrix((np.ones(len(F.data)), F.indices, F.indptr), shape=F.shape)
    cand = sps.triu(P.dot(P.T), k=0 if not fill_diagonal else 1).tocoo()
    r, c, v = [], [], []
    for i, j in zip(cand.row.tolist(), cand.col.tolist()):            # i <= j
        mn, mx = weighted_pair(rows[i], rows[j])
        if mn:
            w = mn / mx
            r += [j] if i == j else [j, i]
            c += [i] if i == j else [i, j]
            v += [w] if i == j else [w, w]
    S = sps.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()
    if fill_diagonal:
        _set_diagonal(S, 1)
    return canonical(S)


def similarity(F, kind, fill_diagonal=True):
    if kind == 'cosine':
        return cosine(F, fill_diagonal)
    if kind == 'cosine-binary':
        return cosine(F, fill_diagonal, assume_binary=True)
    if kind == 'tfidf-cosine':
        return cosine(tfidf(F), fill_diagonal)
    if kind == 'jaccard':
        return jaccard(F, fill_diagonal)
    if kind == 'jaccard-weighted':
        return jaccard_weighted(F, fill_diagonal)
    raise NotImplementedError(kind)


def cross(F_rows, F_cols, kind):
    """The block [rows, cols] of the similarity over the items of F_cols followed by those of F_rows, canonical."""
    F_rows, F_cols = F_rows.tocsr(), F_cols.tocsr()
    if kind == 'jaccard-weighted':
        Fr, rr = _rows(F_rows)
        Fc, rc = _rows(F_cols)
        Pr = sps.csr_matrix((np.ones(Fr.nnz), Fr.indices, Fr.indptr), shape=Fr.shape)
        Pc = sps.csr_matrix((np.ones(Fc.nnz), Fc.indices, Fc.indptr), shape=Fc.shape)
        cand = Pr.dot(Pc.T).tocoo()
        r, c, v = [], [], []
        for j, i in zip(cand.row.tolist(), cand.col.tolist()):        # the row item comes later in the stack: it is j
            mn, mx = weighted_pair(rc[i], rr[j])
            if mn:
                r.append(j)
                c.append(i)
                v.append(mn / mx)
        return canonical(sps.coo_matrix((v, (r, c)), shape=(F_rows.shape[0], F_cols.shape[0])))
    if kind == 'jaccard':
        Pr, Pc = F_rows != 0, F_cols != 0
        S = Pr.astype(np.float64).dot(Pc.T)
        return canonical(_jaccard_divide(S, Pr.getnnz(axis=1), Pc.getnnz(axis=1)))
    if kind == 'tfidf-cosine':
        stack = sps.vstack([F_cols, F_rows], format='csr')
        F_rows, F_cols = tfidf(F_rows, stack), tfidf(F_cols, stack)
    binary = kind == 'cosine-binary'
    if kind not in ('cosine', 'cosine-binary', 'tfidf-cosine'):
        raise NotImplementedError(kind)
    return canonical(normalized(F_rows, binary).dot(normalized(F_cols, binary).T))
