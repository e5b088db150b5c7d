"""NumPy / SciPy restatement of SimilarityAggregation ('SIM') and SimilarityAggregationItemColdStart ('SIM(cs)'): the
scores are SciPy's sparse product `L.dot(B)` (whose summation order the device kernel reproduces bit for bit), classes and
selection are those of tests/i2i_reference.py (`classes`, `select`: class desc, score desc, item asc).  A helper module:
tests/test_sim_host.py pins it against the reference's own lists (tests/golden/sim_*.npz, simcs_*.npz), the GPU tests
compare the device lists and scores with it exactly."""
import numpy as np
import scipy.sparse as sps

import i2i_reference as ref


def product(L, B):
    """Dense fp64 L B by SciPy's csr_matmat: per output entry the products in ascending order of L's stored entries."""
    L, B = sps.csr_matrix(L), sps.csr_matrix(B)
    out = np.asarray(L.dot(B).toarray(), dtype=np.float64)
    return out + 0.0                            # -0 -> +0


def seen_mask(L):
    """Boolean [n_rows x n_cols of L]: the stored entries of every row, zero-valued ones included."""
    L = sps.csr_matrix(L)
    seen = np.zeros(L.shape, dtype=bool)
    rows = np.repeat(np.arange(L.shape[0]), np.diff(L.indptr))
    seen[rows, L.indices] = True
    return seen


def similarity(g):
    """S of a SIM fixture as the model uses it: the stored relations without their diagonal, without explicit zeros."""
    n = int(g['train_shape'][1])
    S = sps.csr_matrix((g['s_val'], (g['s_row'], g['s_col'])), shape=(n, n))
    S.setdiag(0)
    S.eliminate_zeros()
    S.sort_indices()
    return S


def sim_test_matrix(g, implicit=None):
    """CSR of every test entry; zero feedback is kept as a stored zero (seen, no score).  `implicit`: every NONZERO value
    becomes 1 (the reference's get_test_matrix drops zero feedback before its `ones_like`, models.py:197-201)."""
    implicit = bool(g['implicit']) if implicit is None else implicit
    shape = tuple(int(x) for x in g['test_shape'])[:2]
    f = np.asarray(g['test_fdbk'], dtype=np.float64)
    if implicit:
        f = (f != 0).astype(np.float64)
    order = np.lexsort((g['test_item'], g['test_user']))
    u, i, f = g['test_user'][order], g['test_item'][order], f[order]
    indptr = np.r_[0, np.cumsum(np.bincount(u, minlength=shape[0]))]
    return sps.csr_matrix((f, i, indptr), shape=shape)


def sim_lists(g, dense_output=None):
    """(scores, classes, lists) of a sim_* fixture; dense_output overrides the fixture's branch."""
    dense = bool(g['dense_output']) if dense_output is None else dense_output
    S, T = similarity(g), sim_test_matrix(g)
    B = S if dense else S.T.tocsr()
    B.sort_indices()
    scores = product(T, B)
    seen = seen_mask(T)
    topk, fs = int(g['topk']), bool(g['filter_seen'])
    return scores, ref.classes(scores, seen, fs, not dense), ref.select(scores, seen, topk, fs, not dense)


def cold_similarity(g):
    """The cold similarity of a simcs_* fixture in the order the reference stored it (rows not sorted by column: SciPy's
    product, and the device kernel, add in the stored order)."""
    shape = tuple(int(x) for x in g['cold_shape'])
    rows = np.asarray(g['cold_row'], dtype=np.int64)
    assert (rows[1:] >= rows[:-1]).all()
    indptr = np.r_[0, np.cumsum(np.bincount(rows, minlength=shape[0]))]
    return sps.csr_matrix((np.asarray(g['cold_val'], np.float64), np.asarray(g['cold_col'], np.int32), indptr), shape=shape)


def simcs_training(g):
    A = sps.csr_matrix((np.asarray(g['train_val'], np.float64), (g['train_idx'][:, 0], g['train_idx'][:, 1])),
                       shape=tuple(int(x) for x in g['train_shape']))
    A.sum_duplicates()
    if bool(g['implicit']):
        A.data = np.ones_like(A.data)
    return A


def simcs_lists(g):
    """(scores, classes, lists) of a simcs_* fixture: cold items x training users, sparse branch, nothing seen."""
    L = cold_similarity(g)
    B = simcs_training(g).T.tocsr()
    B.sort_indices()
    scores = product(L, B)
    seen = np.zeros(scores.shape, dtype=bool)
    return scores, ref.classes(scores, seen, False, True), ref.select(scores, seen, int(g['topk']), False, True)


def fixture_lists(g):
    return simcs_lists(g) if str(g['model']) == 'SIM(cs)' else sim_lists(g)
