"""Item similarity matrices from item features, built on the device: the reference's `polara/lib/similarity.py`
(`cosine_similarity`, `cosine_tfidf_similarity`, `jaccard_similarity`, `jaccard_similarity_weighted`, `_sim_func`,
`combine_similarity_data` after its feature parsing) on one sparse x sparse product with CSR output (csrc/spgemm.hip).

What runs where.  The per-item and per-label vectors — inverse root norms, idf, entry counts — are O(nnz) work and n numbers:
they are computed on the host with the reference's own NumPy / SciPy expressions (a device `pow` or `log` is not correctly
rounded and would break bit-equality) and applied to the device CSR by pk_csr_scale_f64.  The product F F^T, the Jaccard
epilogues and the diagonal run on the device.  Every result is bit-equal to the reference's matrix made canonical
(`tocsr()`, `sort_indices()`), with one documented exception: `jaccard_similarity` COUNTS the intersection in fp64, where
the reference under SciPy 1.15 multiplies boolean matrices and gets 1 for every count.

Summation order.  SciPy's product adds the terms of an entry in the stored order of the left row.  The reference's
normalisation `diags(norm).dot(F)` is itself a sparse product, and SciPy emits a product's row in the reverse of the order
its columns were first touched: the cosine kinds therefore sum over the labels of an item in the REVERSE of F's stored
order, and the left operand goes to the device with its rows reversed.  F is taken in its stored order (CSR; other formats
are converted with `tocsr()`), duplicates are not summed, as in the reference."""
import numpy as np

KINDS = ('jaccard', 'cosine', 'tfidf-cosine', 'jaccard-weighted')


# ---- host side: arguments and the reference's vectors --------------------------------------------------------------------
def _host_csr(F, what='F'):
    """`F` (SciPy sparse, ndarray or DeviceCSR) as a SciPy CSR in its stored order, checked."""
    from scipy.sparse import csr_matrix, issparse
    from .ops import DeviceCSR
    if isinstance(F, DeviceCSR):
        indptr, indices, values = (F.ops.to_host(x) for x in (F.indptr, F.indices, F.values))
        F = csr_matrix((values, indices, indptr), shape=F.shape)
    elif issparse(F):
        if F.ndim != 2:
            raise ValueError('%s must be a 2-D feature matrix (items x labels), got %d dimensions' % (what, F.ndim))
        F = F.tocsr()
    else:
        F = np.asarray(F)
        if F.ndim != 2:
            raise ValueError('%s must be a 2-D feature matrix (items x labels), got %d dimensions' % (what, F.ndim))
        F = csr_matrix(F)
    if F.dtype != np.float64:
        F = F.astype(np.float64)          # the contract is fp64 features: other types are widened first
    if not np.isfinite(F.data).all():
        raise ValueError('%s holds non-finite values' % what)
    return F


def safe_inverse_root(d):
    """d ** -0.5 where d > 0, else 0 (fp64)."""
    d = np.asarray(d)
    res = np.zeros(len(d), dtype=np.float64)
    np.power(d, -0.5, where=d > 0, out=res)
    return res


def _row_square_sums(F):
    return np.asarray(F.power(2).sum(axis=1)).reshape(-1)


def _idf(F):
    """log((1 + N) / (1 + label frequency)) over the stored entries of F (explicit zeros count, as in the reference)."""
    return np.log((1 + F.shape[0]) / (1 + F.getnnz(axis=0)))


def _reversed_rows(F):
    """(indptr, indices, data) of F with the entries of every row in reverse order."""
    indptr = F.indptr.astype(np.int64)
    n = len(F.indices)
    rows = np.repeat(np.arange(F.shape[0]), np.diff(indptr))
    src = indptr[rows] + indptr[rows + 1] - 1 - np.arange(n)
    return indptr, F.indices[src], F.data[src]


# ---- device side ------------------------------------------------------------------------------------------------------
def _ops(ops):
    if ops is None:
        from .ops import HipOps
        ops = HipOps()
    return ops


def _finish(S, device):
    if device:
        return S
    from scipy.sparse import csr_matrix
    ops = S.ops
    return csr_matrix((ops.to_host(S.values), ops.to_host(S.indices), ops.to_host(S.indptr)), shape=S.shape)


def _scaled(ops, triple, shape, row_scale, col_scale=None):
    indptr, indices, data = triple
    A = ops.csr(indptr, indices, data, shape)
    cs = np.ones(shape[1]) if col_scale is None else col_scale
    return ops.csr_scale(A, row_scale, cs)


def _cosine_operands(ops, F, mode, idf=None):
    """The device CSR of one side of a cosine kind, rows reversed: norm[i] * F[i, k] ('cosine', 'binary': F's own values)
    or norm[i] * idf[k] ('tfidf': every stored entry)."""
    from scipy.sparse import csr_matrix
    if mode == 'tfidf':
        T = csr_matrix((np.take(idf, F.indices), F.indices, F.indptr), shape=F.shape)
        norm = safe_inverse_root(_row_square_sums(T))
        indptr, indices, _ = _reversed_rows(F)
        return _scaled(ops, (indptr, indices, np.ones(len(indices))), F.shape, norm, idf)
    norm = safe_inverse_root(F.getnnz(axis=1) if mode == 'binary' else _row_square_sums(F))
    return _scaled(ops, _reversed_rows(F), F.shape, norm)


def _pattern(F):
    """F != 0 as an fp64 0/1 CSR in F's stored order."""
    P = F.copy()
    P.eliminate_zeros()
    P.data = np.ones(len(P.data))
    return P


def _sorted(F):
    W = F.copy()
    W.sort_indices()
    W.data = W.data.astype(np.float64, copy=False)
    return W


def _device(ops, M):
    return ops.csr(M.indptr, M.indices, M.data, M.shape)


def _build(kind, Fr, Fc, diag, ops, assume_binary=False):
    """The device CSR of the similarity of the items of Fr (rows) to the items of Fc (columns; None: Fr itself)."""
    ops = _ops(ops)
    square = Fc is None
    if kind in ('cosine', 'tfidf-cosine'):
        mode = 'tfidf' if kind == 'tfidf-cosine' else ('binary' if assume_binary else 'cosine')
        idf = None
        if mode == 'tfidf':
            from scipy.sparse import vstack
            idf = _idf(Fr if square else vstack([Fc, Fr], format='csr'))
        L = _cosine_operands(ops, Fr, mode, idf)
        R = L if square else _cosine_operands(ops, Fc, mode, idf)
        return ops.spgemm_csr(L, R.T, diag=diag)
    if kind == 'jaccard':
        Pr = _pattern(Fr)
        Pc = Pr if square else _pattern(Fc)
        L = _device(ops, Pr)
        R = L if square else _device(ops, Pc)
        return ops.spgemm_csr(L, R.T, epilogue='jaccard', diag=diag, nf_rows=Pr.getnnz(axis=1).astype(np.float64),
                              nf_cols=Pc.getnnz(axis=1).astype(np.float64))
    if kind == 'jaccard-weighted':
        L = _device(ops, _sorted(Fr))
        R = L if square else _device(ops, _sorted(Fc))
        return ops.spgemm_csr(L, R.T, op='min', epilogue='wjaccard', diag=diag, col_features=R, rectangular=not square)
    raise NotImplementedError('unknown similarity kind %r (known: %s)' % (kind, ', '.join(KINDS)))


def _kind(kind):
    if not isinstance(kind, str) or kind.lower() not in KINDS:
        raise NotImplementedError('unknown similarity kind %r (known: %s)' % (kind, ', '.join(KINDS)))
    return kind.lower()


# ---- public functions ---------------------------------------------------------------------------------------------------
def cosine_similarity(F, fill_diagonal=True, assume_binary=False, device=False, ops=None):
    """Cosine similarity of the rows of F.  `assume_binary` takes the entry count of a row for its squared norm (the values
    themselves are used as they are, as in the reference).  An item without features gets an all-zero row and, under
    `fill_diagonal`, a 1 on its diagonal.  Returns a canonical SciPy CSR, or the DeviceCSR with `device=True`."""
    return _finish(_build('cosine', _host_csr(F), None, bool(fill_diagonal), ops, assume_binary), device)


def cosine_tfidf_similarity(F, fill_diagonal=True, device=False, ops=None):
    """Cosine similarity of the idf-weighted pattern of F: every stored entry of label k counts log((1 + N) / (1 + freq_k))."""
    return _finish(_build('tfidf-cosine', _host_csr(F), None, bool(fill_diagonal), ops), device)


def jaccard_similarity(F, fill_diagonal=True, device=False, ops=None):
    """|i and j| / |i or j| over the nonzero pattern of F, the intersection counted in fp64 (see the module docstring)."""
    return _finish(_build('jaccard', _host_csr(F), None, bool(fill_diagonal), ops), device)


def jaccard_similarity_weighted(F, fill_diagonal=True, device=False, ops=None):
    """sum_k min(F_ik, F_jk) / sum_k max(F_ik, F_jk), stored where the numerator is nonzero; the denominator is added up in
    the reference's order for the pair (min(i, j), max(i, j)).  Without `fill_diagonal` the diagonal is 1 where the row's
    numerator with itself is nonzero and is not stored otherwise."""
    return _finish(_build('jaccard-weighted', _host_csr(F), None, bool(fill_diagonal), ops), device)


def similarity(F, kind, fill_diagonal=True, device=False, ops=None):
    """The similarity of the given kind, by the reference's names: 'jaccard', 'cosine', 'tfidf-cosine', 'jaccard-weighted'."""
    return _finish(_build(_kind(kind), _host_csr(F), None, bool(fill_diagonal), ops), device)


def cross_similarity(F_rows, F_cols, kind, assume_binary=False, device=False, ops=None):
    """The block [rows, cols] of the similarity of `kind` over the items of F_cols followed by the items of F_rows, without
    any diagonal treatment: what `cold_relations_matrices` wants for SIM(cs) (cold items x training items).  The idf of
    'tfidf-cosine' is taken over the stacked matrix; `assume_binary` is that of `cosine_similarity` (kind 'cosine' only)."""
    kind = _kind(kind)
    Fr, Fc = _host_csr(F_rows, 'F_rows'), _host_csr(F_cols, 'F_cols')
    if Fr.shape[1] != Fc.shape[1]:
        raise ValueError('F_rows has %d labels, F_cols %d' % (Fr.shape[1], Fc.shape[1]))
    return _finish(_build(kind, Fr, Fc, False, ops, bool(assume_binary)), device)


def combine_similarity(mats, weights=None):
    """The weighted sum of similarity matrices (default: equal weights 1 / len(mats)) with the diagonal set to 1 and values
    above 1 clipped to 1 — the tail of the reference's combine_similarity_data.  Host-side SciPy: its addition is the
    contract.  `mats`: a sequence, or a dict with `weights` a dict over the same keys.  Returns a CSC matrix."""
    import warnings
    from scipy.sparse import SparseEfficiencyWarning, csc_matrix
    if isinstance(mats, dict):
        keys = list(mats)
        weights = None if weights is None else [weights[k] for k in keys] if isinstance(weights, dict) else list(weights)
        mats = [mats[k] for k in keys]
    mats = list(mats)
    if not mats:
        raise ValueError('combine_similarity: no matrices given')
    if weights is None:
        weights = [1.0 / len(mats)] * len(mats)
    if len(weights) != len(mats):
        raise ValueError('combine_similarity: %d matrices, %d weights' % (len(mats), len(weights)))
    shape = mats[0].shape
    if len(shape) != 2 or shape[0] != shape[1] or any(m.shape != shape for m in mats):
        raise ValueError('combine_similarity: the matrices must be square and of one shape')
    total = csc_matrix(shape)
    for w, m in zip(weights, mats):
        total += w * m
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', category=SparseEfficiencyWarning)
        total.setdiag(1)
    total.data[total.data > 1] = 1
    return total
