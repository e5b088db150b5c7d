"""NumPy / SciPy restatement of the neighbour pass without an image (pk_spsp_knn_f64: the contract of
include/polara_hip.h, csrc/uknn.hip) and of what polara_amd.knn builds on it: UserKNNModel and the `gram = 'sparse'` route
of ItemKNNModel and RP3BetaModel.  g is SciPy's sparse product (tests/sim_reference.py: the summation order the kernel
reproduces), the weights and the selection are those of tests/knn_reference.py applied to a rectangular g with an excluded
column per row; lists are selected with tests/i2i_reference.py.  The last part is a dense textbook UserKNN that shares
nothing with the rest."""
import numpy as np
import scipy.sparse as sps

import knn_reference as knn_ref
import sim_reference as sim_ref

SCALE, COSINE, TANIMOTO = knn_ref.SCALE, knn_ref.COSINE, knn_ref.TANIMOTO
U, gamma = knn_ref.U, knn_ref.gamma
FIXTURES, training, training_matrix, test_rows = knn_ref.FIXTURES, knn_ref.training, knn_ref.training_matrix, knn_ref.test_rows


def canonical(A):
    """fp64 SciPy CSR copy with sorted columns (stored zeros stay)."""
    A = sps.csr_matrix(A, dtype=np.float64, copy=True)
    A.sort_indices()
    return A


def transposed(A):
    """The canonical CSR of A^T: per row (a column of A) the entries in ascending row of A."""
    return canonical(canonical(A).T.tocsr())


# ---- the pass ----------------------------------------------------------------------------------------------------------
def product(L, B):
    """Dense g [n_rows x n_cols] = L B in SciPy's order, -0 as +0."""
    return sim_ref.product(L, B)


def ranked(g, kind, row, col, shrink, exclude=None):
    """(w, per row the candidate columns best first) for a rectangular g: candidate = not the row's excluded column (when
    `exclude` is given and >= 0), g != 0, w finite and != 0; order = w descending, then column ascending."""
    g = np.asarray(g, dtype=np.float64)
    w = knn_ref.weights(g, kind, row, col, shrink)
    cand = (g != 0) & np.isfinite(w) & (w != 0)
    if exclude is not None:
        for r, c in enumerate(np.asarray(exclude)):
            if 0 <= c < g.shape[1]:
                cand[r, c] = False
    order = []
    for r in range(g.shape[0]):
        cols = np.flatnonzero(cand[r])
        order.append(cols[np.argsort(-w[r, cols], kind='stable')])
    return w, order


def slots(g, kind, row, col, shrink, K, normalize, exclude=None):
    """(count int32 [n_rows], idx int32 [n_rows x K], val fp64 [n_rows x K]) of the contract."""
    return knn_ref.prune_ranked(ranked(g, kind, row, col, shrink, exclude), K, normalize)


def slots_csr(count, idx, val, n_cols):
    indptr = np.concatenate(([0], np.cumsum(count, dtype=np.int64)))
    stored = idx >= 0
    return sps.csr_matrix((val[stored], idx[stored].astype(np.int32), indptr), shape=(len(count), n_cols))


# ---- UserKNN -----------------------------------------------------------------------------------------------------------
def squared_sums(keys, vals, n):
    return np.bincount(keys, weights=vals * vals, minlength=n)


def row_norms(A):
    """q_v = sum_i a_vi^2 by np.bincount over the canonical storage order."""
    A = canonical(A)
    return squared_sums(np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), A.data, A.shape[0])


def similarity_vectors(similarity, q_rows, q_cols, alpha):
    if similarity == 'cosine':
        return COSINE, knn_ref.power(q_rows, 1.0 - alpha), knn_ref.power(q_cols, alpha)
    return TANIMOTO, q_rows, q_cols


def user_neighbours(L, X, similarity, neighbours, shrink=0.0, alpha=0.5, normalize=False, exclude=None, g=None):
    """N_L (SciPy CSR [rows of L x users of X]): the pruned rows of L X^T, the target user being the row.  `g`: the
    product L X^T when the caller already has it."""
    L, X = canonical(L), canonical(X)
    kind, row, col = similarity_vectors(similarity, row_norms(L), row_norms(X), alpha)
    g = product(L, transposed(X)) if g is None else g
    return slots_csr(*slots(g, kind, row, col, shrink, neighbours, normalize, exclude), X.shape[0])


def user_knn_weights(X, similarity, neighbours, shrink=0.0, alpha=0.5, normalize=False, g=None):
    """N over the training users: no user is its own neighbour."""
    return user_neighbours(X, X, similarity, neighbours, shrink, alpha, normalize, np.arange(X.shape[0]), g)


def scores(N_test, X):
    """Dense N_test X in SciPy's order."""
    return sim_ref.product(N_test, canonical(X))


# ---- gram = 'sparse' ---------------------------------------------------------------------------------------------------
def item_knn_sparse_weights(A, similarity, neighbours, shrink=0.0, alpha=0.5, normalize=False):
    """W of ItemKNNModel(gram='sparse'): g = A^T A summed per entry in ascending user, q the squared column norms by
    np.bincount over A's storage order; the target rows pruned, then transposed."""
    A = canonical(A)
    n = A.shape[1]
    q = squared_sums(A.indices, A.data, n)
    kind, row, col = similarity_vectors(similarity, q, q, alpha)
    g = product(transposed(A), A)
    W = slots_csr(*slots(g, kind, row, col, shrink, neighbours, normalize, np.arange(n)), n).T.tocsr()
    W.sort_indices()
    return W


def rp3_sparse_weights(A, alpha, beta, neighbours, normalize=False):
    """W of RP3BetaModel(gram='sparse'): the rows of r_i (X'^T X')[i, j] c_j pruned directly, without the diagonal (as
    the image route, whose pass never keeps j = i)."""
    X, r, c = knn_ref.rp3_parts(A, alpha, beta)
    X = canonical(X)
    g = product(transposed(X), X)
    return slots_csr(*slots(g, SCALE, r, c, 0.0, neighbours, normalize, np.arange(X.shape[1])), X.shape[1])


# ---- the textbook (dense, independent of the above) --------------------------------------------------------------------
def textbook_user_knn(A, similarity, shrink=0.0, alpha=0.5):
    """Dense N[u, v] before pruning, diagonal included: u the target."""
    X = np.asarray(A.todense(), dtype=np.float64)
    G = X @ X.T
    q = np.einsum('ij,ij->i', X, X)
    with np.errstate(divide='ignore', invalid='ignore'):
        if similarity == 'cosine':
            return G / (np.outer(q ** (1.0 - alpha), q ** alpha) + shrink)
        return G / (q[:, None] + q[None, :] - G + shrink)
