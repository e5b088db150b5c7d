"""NumPy restatement of the top-K pruning pass (pk_knn_prune_f64: the contract of include/polara_hip.h, csrc/knn.hip) and
of what polara_amd.knn builds around it: the scale vectors and the weights W of ItemKNNModel and RP3BetaModel from a host
Gram matrix.  NumPy's element-wise fp64 operations round every product, sum, difference and quotient on its own and its
division is the correctly rounded one, as the contract demands.  Fixtures and test rows are those of
tests/ease_reference.py; scores are summed in SciPy's order (tests/sim_reference.py) and lists are selected and compared
with tests/i2i_reference.py."""
import numpy as np
import scipy.sparse as sps

import ease_reference as ease_ref
import sim_reference as sim_ref
import slim_reference as slim_ref

FIXTURES = ease_ref.FIXTURES
training, training_matrix, test_rows = ease_ref.training, ease_ref.training_matrix, ease_ref.test_rows
sized_training, gram = slim_ref.sized_training, slim_ref.gram
SCALE, COSINE, TANIMOTO = 0, 1, 2
U = 2.0 ** -53


def gamma(m):
    """gamma_m = m u / (1 - m u): the relative error bound of a sum of m non-negative rounded products."""
    return m * U / (1.0 - m * U)


# ---- the pruning pass ------------------------------------------------------------------------------------------------
def weights(G, kind, row, col, shrink):
    """w [n x n] of the contract, operation by operation (0/0 and x/0 give NaN / inf silently, as on the device)."""
    G = np.asarray(G, dtype=np.float64)
    r, c = np.asarray(row, dtype=np.float64)[:, None], np.asarray(col, dtype=np.float64)[None, :]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        if kind == SCALE:
            return (G * r) * c
        if kind == COSINE:
            return G / (r * c + shrink)
        if kind == TANIMOTO:
            return G / (((r + c) - G) + shrink)
    raise ValueError('unknown kind %r' % (kind,))


def ranked(G, kind, row, col, shrink):
    """(w, per row the candidate columns best first): candidate = off the diagonal, g != 0, w finite and != 0; order = w
    descending, then column ascending (a stable sort of the candidates, which are listed in ascending column order)."""
    G = np.asarray(G, dtype=np.float64)
    n = G.shape[0]
    w = weights(G, kind, row, col, shrink)
    cand = (G != 0) & np.isfinite(w) & (w != 0)
    cand[np.arange(n), np.arange(n)] = False
    order = []
    for i in range(n):
        cols = np.flatnonzero(cand[i])
        order.append(cols[np.argsort(-w[i, cols], kind='stable')])
    return w, order


def sequential_abs_sum(x):
    """((+0.0 + |x_0|) + |x_1|) + ...: np.cumsum accumulates from left to right, one rounded addition per element."""
    return float(np.cumsum(np.abs(x))[-1]) if len(x) else 0.0


def prune_ranked(rank, K, normalize):
    """(count int32 [n], idx int32 [n x K], val fp64 [n x K]) of the contract from `ranked`'s output."""
    w, order = rank
    n = w.shape[0]
    count = np.zeros(n, dtype=np.int32)
    idx = np.full((n, K), -1, dtype=np.int32)
    val = np.zeros((n, K), dtype=np.float64)
    for i in range(n):
        kept = np.sort(order[i][:K])
        wk = w[i, kept]
        if normalize:
            s = sequential_abs_sum(wk)
            if np.isfinite(s) and s != 0:
                wk = wk / s
        count[i] = len(kept)
        idx[i, :len(kept)] = kept
        val[i, :len(kept)] = wk
    return count, idx, val


def prune(G, kind, row, col, shrink, K, normalize):
    return prune_ranked(ranked(G, kind, row, col, shrink), K, normalize)


def slots_csr(count, idx, val):
    """The canonical SciPy CSR [n x n] of the slots: indptr the cumulative counts, the non-pad slots in row-major order."""
    n = len(count)
    indptr = np.concatenate(([0], np.cumsum(count, dtype=np.int64)))
    stored = idx >= 0
    return sps.csr_matrix((val[stored], idx[stored].astype(np.int32), indptr), shape=(n, n))


# ---- the vectors and weights of the models ---------------------------------------------------------------------------
def power(v, exponent):
    """np.sqrt for an exponent of exactly 0.5, np.power otherwise."""
    v = np.asarray(v, dtype=np.float64)
    return np.sqrt(v) if exponent == 0.5 else np.power(v, float(exponent))


def inverse_power(v, exponent):
    """v ** -exponent over the positive entries (np.power of exactly those), 0 elsewhere."""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(v.shape)
    out[v > 0] = np.power(v[v > 0], -float(exponent))
    return out


def item_knn_slots(G, similarity, neighbours, shrink=0.0, alpha=0.5, normalize=False):
    """The slots of the pruned TARGET rows: row = q^(1 - alpha), col = q^alpha for the cosine, q and q for jaccard."""
    q = np.ascontiguousarray(np.diagonal(G))
    if similarity == 'cosine':
        return prune(G, COSINE, power(q, 1.0 - alpha), power(q, alpha), shrink, neighbours, normalize)
    return prune(G, TANIMOTO, q, q, shrink, neighbours, normalize)


def item_knn_weights(G, similarity, neighbours, shrink=0.0, alpha=0.5, normalize=False):
    """W (SciPy CSR, canonical): W[i, j] the weight of source i for target j — the transpose of the pruned target rows."""
    W = slots_csr(*item_knn_slots(G, similarity, neighbours, shrink, alpha, normalize)).T.tocsr()
    W.sort_indices()
    return W


def rp3_parts(A, alpha, beta):
    """(X', r, c) for the canonical SciPy CSR A >= 0: X' = diag(d_u^(-alpha / 2)) A^alpha with a^alpha taken over the
    DISTINCT stored values when alpha != 1 and the values are not all 1, r = d_i^(-alpha), c = pop^(-beta)."""
    A = sps.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    n_users, n_items = A.shape
    rows = np.repeat(np.arange(n_users), np.diff(A.indptr))
    d_user = np.bincount(rows, weights=A.data, minlength=n_users)
    d_item = np.bincount(A.indices, weights=A.data, minlength=n_items)
    pop = np.bincount(A.indices[A.data > 0], minlength=n_items).astype(np.float64)
    vals = A.data
    if alpha != 1.0 and len(vals) and not (vals == 1.0).all():
        distinct, where = np.unique(vals, return_inverse=True)
        vals = np.where(distinct == 0, 0.0, np.power(distinct, float(alpha)))[where]      # a stored 0 is no walk
    X = sps.csr_matrix((inverse_power(d_user, alpha / 2.0)[rows] * vals, A.indices.copy(), A.indptr.copy()), shape=A.shape)
    return X, inverse_power(d_item, alpha), inverse_power(pop, beta)


def rp3_weights(G, A, alpha, beta, neighbours, normalize=False):
    """W (SciPy CSR, canonical) from the Gram matrix G of X' (rp3_parts): the rows of r_i G[i, j] c_j pruned directly."""
    _, r, c = rp3_parts(A, alpha, beta)
    return slots_csr(*prune(G, SCALE, r, c, 0.0, neighbours, normalize))


def scores(W, T):
    """Dense scores T W in the order of SciPy's sparse product (the order of the device's scoring pass)."""
    return sim_ref.product(T, sps.csr_matrix(W))


# ---- textbook expressions (dense, independent of the above) ----------------------------------------------------------
def textbook_item_knn(A, similarity, shrink=0.0, alpha=0.5):
    """Dense W[i, j] before pruning, diagonal included."""
    X = np.asarray(A.todense(), dtype=np.float64)
    G = X.T @ X
    q = np.diag(G)
    with np.errstate(divide='ignore', invalid='ignore'):
        if similarity == 'cosine':
            return G / (np.outer(q ** alpha, q ** (1.0 - alpha)) + shrink)
        return G / (q[:, None] + q[None, :] - G + shrink)


def textbook_rp3(A, alpha, beta):
    """Dense W[i, j] = pop_j^(-beta) sum_u (a_ui / d_i)^alpha (a_uj / d_u)^alpha, zero where a count is zero."""
    X = np.asarray(A.todense(), dtype=np.float64)
    d_u, d_i, pop = X.sum(1), X.sum(0), (X > 0).sum(0).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        p_iu = np.where(d_i[:, None] > 0, (X.T / d_i[:, None]) ** alpha, 0.0)
        p_uj = np.where(d_u[:, None] > 0, (X / d_u[:, None]) ** alpha, 0.0)
        disc = np.where(pop > 0, pop ** -float(beta), 0.0)
    p_iu[X.T == 0] = 0.0          # 0 ** 0 = 1 is no walk
    p_uj[X == 0] = 0.0
    return (p_iu @ p_uj) * disc[None, :]
