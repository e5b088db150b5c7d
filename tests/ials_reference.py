"""TEST-ONLY NumPy restatement of implicit ALS (polara_amd/ials.py, csrc/ials.hip): the half-step as a per-row loop with A and b
formed in storage order, the fit, the objective computed densely and by the trace formula, the error bound of a half-step, and
the CPU double of the iALS operators on top of tests/numpy_ops.py.  Never imported by the package."""
import numpy as np
import scipy.sparse as sps
import torch

from numpy_ops import NpCSR, NumpyOps
from polara_amd import ials
from pmf_reference import top_lists  # noqa: F401  (shared with the iALS tests)

MAX_RANK = 128
EPS = 2.0 ** -53


class NotPositiveDefinite(ValueError):
    pass


def chol_solve(A, b):
    """x = A^-1 b by a plain column Cholesky (lower triangle of A only), forward and back substitution"""
    k = len(b)
    L = np.zeros((k, k))
    for j in range(k):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise NotPositiveDefinite(j)
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    z = np.zeros(k)
    for j in range(k):
        z[j] = (b[j] - L[j, :j] @ z[:j]) / L[j, j]
    x = np.zeros(k)
    for j in range(k - 1, -1, -1):
        x[j] = (z[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


def lapack_solve(A, b):
    return np.linalg.solve(A, b)


def as_csr(C):
    C = C.m if hasattr(C, 'm') else C
    C = sps.csr_matrix(C)
    return C.indptr, C.indices, np.asarray(C.data, dtype=np.float64), C.shape


def row_system(indices, conf, Y, G, lam, skip=None):
    """(A_u, b_u) of one row, the sums in storage order; skip: position of an interaction to leave out"""
    k = Y.shape[1]
    A = G + lam * np.eye(k)
    b = np.zeros(k)
    for p, (i, c) in enumerate(zip(indices, conf)):
        if p == skip:
            continue
        y = Y[i]
        A = A + (c - 1.0) * np.outer(y, y)
        b = b + c * y
    return A, b


def half_step(C, Y, G, lam, solve=chol_solve):
    """X [n_rows x k]: x_u = A_u^-1 b_u for every row of C; an empty row gives zeros.  Raises NotPositiveDefinite with
    (count, first row) when `solve` refuses rows; their x_u are zeros in the exception's `X`."""
    indptr, indices, data, shape = as_csr(C)
    k = Y.shape[1]
    X = np.zeros((shape[0], k))
    bad = []
    for u in range(shape[0]):
        lo, hi = indptr[u], indptr[u + 1]
        if hi == lo:
            continue
        A, b = row_system(indices[lo:hi], data[lo:hi], Y, G, lam)
        try:
            X[u] = solve(A, b)
        except NotPositiveDefinite:
            bad.append(u)
    if bad:
        err = NotPositiveDefinite('iALS half-step: %d row(s) whose normal equations are not positive definite, the first is row %d'
                                  % (len(bad), bad[0]))
        err.X, err.count, err.first = X, len(bad), bad[0]
        raise err
    return X


def objective(C, X, Y, lam):
    """sum over all pairs of w (p - x.y)^2 + lam (|X|^2 + |Y|^2), computed densely"""
    indptr, indices, data, shape = as_csr(C)
    S = X @ Y.T
    W = np.ones(shape)
    P = np.zeros(shape)
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    W[rows, indices] = data
    P[rows, indices] = 1.0
    return float((W * (P - S) ** 2).sum() + lam * ((X * X).sum() + (Y * Y).sum()))


def objective_by_traces(C, X, Y, lam):
    """the same by  tr(X^T X Y^T Y) + sum_nz [c (1 - s)^2 - s^2] + lam (tr X^T X + tr Y^T Y)"""
    indptr, indices, data, shape = as_csr(C)
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    s = np.einsum('ij,ij->i', X[rows], Y[indices])
    GX, GY = X.T @ X, Y.T @ Y
    return float((GX * GY).sum() + (data * (1.0 - s) ** 2 - s * s).sum() + lam * (np.trace(GX) + np.trace(GY)))


def fit(C, rank, lam, num_epochs, seed=None, init=None, solve=chol_solve, loss_history=None):
    """(X, Y) after `num_epochs` times (user half-step, item half-step) from `ials.initial_factors`"""
    C = sps.csr_matrix(C.m if hasattr(C, 'm') else C)
    Ct = sps.csr_matrix(C.T)
    Ct.sort_indices()
    X0, Y0 = ials.initial_factors(C.shape[0], C.shape[1], rank, seed) if init is None else init
    X, Y = np.array(X0, dtype=np.float64), np.array(Y0, dtype=np.float64)
    for _ in range(int(num_epochs)):
        X = half_step(C, Y, Y.T @ Y, lam, solve)
        if loss_history is not None:
            loss_history.append(objective_by_traces(C, X, Y, lam))
        Y = half_step(Ct, X, X.T @ X, lam, solve)
        if loss_history is not None:
            loss_history.append(objective_by_traces(C, X, Y, lam))
    return X, Y


def row_bounds(C, Y, G, lam, X):
    """per row of C the bound on |x^_u - x_u|_2 of a backward-stable half-step in fp64 against the reference solve `X`:
        4 kappa_2(A_u) eps [ (n + 2) S_A / |A_u|_2 + k (3 k + 1) + n S_b / |b_u|_2 ] |x_u|_2,
    S_A = |G|_2 + lam + sum |c - 1| |y_i|^2,  S_b = sum c |y_i|,  n the entries of the row — the rounding of forming A, Higham's
    Cholesky backward error, the rounding of forming b; 4 = 2 (the reference solve's own error of the same class) x 2
    (first-order slack).  0 for an empty row."""
    indptr, indices, data, shape = as_csr(C)
    k = Y.shape[1]
    g2 = np.linalg.norm(G, 2)
    ynorm = np.linalg.norm(Y, axis=1)
    out = np.zeros(shape[0])
    for u in range(shape[0]):
        lo, hi = indptr[u], indptr[u + 1]
        n = hi - lo
        if n == 0:
            continue
        idx, c = indices[lo:hi], data[lo:hi]
        A, b = row_system(idx, c, Y, G, lam)
        sv = np.linalg.svd(A, compute_uv=False)
        S_A = g2 + lam + (np.abs(c - 1.0) * ynorm[idx] ** 2).sum()
        S_b = (c * ynorm[idx]).sum()
        bracket = (n + 2) * S_A / sv[0] + k * (3 * k + 1) + n * S_b / np.linalg.norm(b)
        out[u] = 4.0 * (sv[0] / sv[-1]) * EPS * bracket * np.linalg.norm(X[u])
    return out


# ---- the CPU double of the iALS operators ----------------------------------------------------------------------------------
class NpCSRValues(NpCSR):
    """NpCSR that also carries its stored values as a tensor, like a DeviceCSR"""

    def __init__(self, indptr, indices, values, shape):
        super().__init__(indptr, indices, values, shape)
        self.values = torch.from_numpy(np.asarray(values, dtype=np.float64))

    @property
    def T(self):
        if self._T is None:
            t = self.m.T.tocsr()
            t.sort_indices()
            self._T = NpCSRValues(t.indptr, t.indices, t.data, t.shape)
            self._T._T = self
        return self._T


class IALSNumpyOps(NumpyOps):
    """NumpyOps plus what polara_amd/ials.py asks of HipOps (same semantics on CPU tensors)."""
    solve = staticmethod(chol_solve)

    def ials_max_rank(self):
        return MAX_RANK

    def tile_norm_bound(self, V):
        """NumpyOps' bound with a copy at the end: for a catalogue of one tile (<= 32 items, as in these tests) its strided
        one-element view keeps a negative stride, which torch refuses"""
        nb = (np.linalg.norm(V.numpy(), axis=1) * (1 + 1e-6)).astype(np.float32)
        return torch.from_numpy(np.maximum.accumulate(nb[::-1])[::-1][::32].copy())

    def csr_values_host(self, A):
        return np.array(A.m.data, dtype=np.float64)

    def csr_replace_values(self, A, values, drop_zeros=False):
        values = np.ascontiguousarray(values, dtype=np.float64)
        m = A.m
        if values.shape != (m.nnz,):
            raise ValueError('csr_replace_values: %s values for %d stored entries' % (values.shape, m.nnz))
        keep = values != 0 if drop_zeros else np.ones(len(values), dtype=bool)
        csum = np.concatenate(([0], np.cumsum(keep, dtype=np.int64)))
        return NpCSRValues(csum[m.indptr], m.indices[keep], values[keep], A.shape)

    def csr_scale(self, A, row_scale, col_scale):
        m = A.m
        rows = np.repeat(np.arange(A.shape[0]), np.diff(m.indptr))
        return NpCSRValues(m.indptr, m.indices, (np.asarray(row_scale)[rows] * m.data) * np.asarray(col_scale)[m.indices], A.shape)

    def ials_half_step(self, Cm, Y, regularization, out=None, G=None, row_order=None):
        k = int(Y.shape[1])
        if k < 1 or k > MAX_RANK:
            raise ValueError('iALS: rank %d outside 1..%d' % (k, MAX_RANK))
        Yn = Y.numpy()
        Gn = Yn.T @ Yn if G is None else G.numpy()
        X = torch.empty(Cm.shape[0], k, dtype=torch.float64) if out is None else out
        try:
            X.copy_(torch.from_numpy(half_step(Cm, Yn, Gn, float(regularization), self.solve)))
        except NotPositiveDefinite as err:
            X.copy_(torch.from_numpy(err.X))
            raise ValueError(str(err) + ' (their factors are set to zero)')
        return X

    def ials_loss(self, Cm, X, Y, regularization, GX=None, GY=None):
        return objective_by_traces(Cm, X.numpy(), Y.numpy(), float(regularization))


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def ratings_matrix(seed, n_users, n_items, density):
    """(users, items, ratings 2..5 times {0.5, 1, 3}) in row-major order: every confidence log2(rating) is > 0"""
    rng = np.random.RandomState(seed)
    mask = rng.rand(n_users, n_items) < density
    u, i = np.nonzero(mask)
    r = rng.randint(2, 6, size=len(u)).astype(np.float64)
    return u.astype(np.int64), i.astype(np.int64), r


def model_data(u, i, r, n_users, n_items, seed=0, holdout=True):
    """ArrayData of the triplets; the holdout is one stored entry per user that has at least two"""
    from polara_amd.data import ArrayData
    if not holdout:
        return ArrayData((u, i, r), n_users=n_users, n_items=n_items, fields=('userid', 'itemid', 'rating'))
    rng = np.random.RandomState(seed)
    first = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
    counts = np.diff(np.r_[first, len(u)])
    pick = first[counts >= 2] + (rng.rand((counts >= 2).sum()) * counts[counts >= 2]).astype(np.int64)
    keep = np.ones(len(u), dtype=bool)
    keep[pick] = False
    return ArrayData((u[keep], i[keep], r[keep]), n_users=n_users, n_items=n_items, holdout=(u[pick], i[pick], r[pick]),
                     fields=('userid', 'itemid', 'rating'))


# ---- the inputs of the half-step tests ---------------------------------------------------------------------------------------
CONFIDENCES = np.array([0.25, 0.5, 1.0, 1.5, 2.32, 5.0])
WIDE_LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 257, 1000]


def confidence_matrix(kind):
    """'wide': 40 x 1 100, the row lengths of WIDE_LENGTHS (the K = 4 tail, the staging-chunk tail whatever the chunk is,
    several chunks, the empty row) and the rest random <= 20;  'tall': 3 000 x 16 — more rows than one wave of workgroups;
    'narrow': 30 x 12 — fewer columns than the rank it is used at (16): G is singular there."""
    n_rows, n_cols, seed = {'wide': (40, 1100, 11), 'tall': (3000, 16, 12), 'narrow': (30, 12, 13)}[kind]
    rng = np.random.RandomState(seed)
    if kind == 'wide':
        lengths = np.array(WIDE_LENGTHS + list(rng.randint(0, 21, size=n_rows - len(WIDE_LENGTHS))))
    else:
        lengths = rng.randint(0, n_cols + 1, size=n_rows)
        lengths[:2] = (0, n_cols)
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    indices = np.concatenate([np.sort(rng.permutation(n_cols)[:n]) for n in lengths] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    data = CONFIDENCES[rng.randint(len(CONFIDENCES), size=len(indices))]
    return sps.csr_matrix((data, indices, indptr), shape=(n_rows, n_cols))


def item_block(n_cols, rank, seed=0):
    return np.random.RandomState(1000 * rank + seed).normal(scale=0.3, size=(n_cols, rank))


def dropped_interaction_margin(C, Y, G, lam, X, bounds):
    """the smallest over the non-empty rows of |x(one interaction dropped) - x| / bound — the last interaction of the row is
    the one left out: how far outside the tolerance a kernel that loses a single term lands"""
    indptr, indices, data, shape = as_csr(C)
    worst = np.inf
    for u in range(shape[0]):
        lo, hi = indptr[u], indptr[u + 1]
        if hi == lo:
            continue
        A, b = row_system(indices[lo:hi], data[lo:hi], Y, G, lam, skip=hi - lo - 1)
        x = np.linalg.solve(A, b) if hi - lo > 1 else np.zeros(Y.shape[1])
        worst = min(worst, np.linalg.norm(x - X[u]) / bounds[u])
    return worst


# ---- the inputs of the model tests -------------------------------------------------------------------------------------------
LAMBDA = 0.01
TOPK = 10
MODEL_CASES = {                     # name: (n_users, n_items, rank, epochs, density, seed)
    'r7': (37, 29, 7, 4, 0.2, 1),
    'r16': (60, 45, 16, 4, 0.15, 2),
    'r17': (50, 40, 17, 3, 0.12, 3),
    'r50': (300, 120, 50, 3, 0.08, 4),
}
_cases = {}


def model_case(name):
    """The seeded input of one model test and its restatements, computed once and never written to: feedback r ** m with r a
    rating 2..5 and m in {0.5, 1, 3}, so that the default confidence log2(feedback) is log2(r) times {0.5, 1, 3}; one entry per
    user held out; `X`, `Y`, `loss` the Cholesky statement's factors and objective per half-step, `d` the largest relative
    distance of its factors to those of the statement with np.linalg.solve; `lists` / `gaps` the top lists of the test users
    (seen items masked) and the smallest adjacent gap among their top TOPK + 1 scores."""
    if name in _cases:
        return _cases[name]
    n_users, n_items, rank, epochs, density, seed = MODEL_CASES[name]
    u, i, r = ratings_matrix(seed, n_users, n_items, density)
    f = r ** np.array([0.5, 1.0, 3.0])[np.random.RandomState(seed + 100).randint(3, size=len(r))]
    data = model_data(u, i, f, n_users, n_items, seed)
    tu, ti, tf = data.training
    C = sps.csr_matrix((np.log2(tf), (tu, ti)), shape=(n_users, n_items))
    C.sort_indices()
    loss = []
    X, Y = fit(C, rank, LAMBDA, epochs, seed=seed, loss_history=loss)
    X2, Y2 = fit(C, rank, LAMBDA, epochs, seed=seed, solve=lapack_solve)
    d = max(rel_distance(X2, X), rel_distance(Y2, Y))
    test_users = np.unique(data.test.holdout.userid)
    lists, gaps = lists_and_gaps(X[test_users] @ Y.T, (np.searchsorted(test_users, tu[np.isin(tu, test_users)]), ti[np.isin(tu, test_users)]))
    case = dict(name=name, n_users=n_users, n_items=n_items, rank=rank, epochs=epochs, seed=seed, triplets=(u, i, f), C=C, X=X, Y=Y,
                loss=np.array(loss), d=d, test_users=test_users, lists=lists, gaps=gaps)
    for a in (X, Y, lists, gaps):
        a.setflags(write=False)
    _cases[name] = case
    return case


def rel_distance(A, B):
    return float(np.linalg.norm(A - B) / np.linalg.norm(B))


def lists_and_gaps(scores, seen):
    """(top TOPK lists with `seen` = (rows, cols) masked, per row the smallest gap between adjacent scores among its top TOPK + 1)"""
    s = scores.copy()
    s[seen] = -np.inf
    lists = top_lists(scores, TOPK, seen=seen)
    top = -np.sort(-s, axis=1)[:, :TOPK + 1]
    return lists, np.min(top[:, :-1] - top[:, 1:], axis=1)


def model_for(case, ops, cls=None, data=None, **kwargs):
    cls = ials.ImplicitALS if cls is None else cls
    u, i, f = case['triplets']
    m = cls(model_data(u, i, f, case['n_users'], case['n_items'], case['seed']) if data is None else data, seed=case['seed'], ops=ops,
            **kwargs)
    m.verbose = False
    m.rank, m.num_epochs, m.regularization, m.topk = case['rank'], case['epochs'], LAMBDA, TOPK
    return m


def check_lists(recs, lists, gaps, min_gap=1e-9, max_left_out=0.05):
    """equal lists on every row whose restatement separates its top TOPK + 1 scores by more than `min_gap` (the project's
    convention); at most `max_left_out` of the rows may be left out"""
    clear = gaps > min_gap
    assert recs.shape == lists.shape and (~clear).mean() <= max_left_out
    assert np.array_equal(recs[clear], lists[clear])


def warm_case(name='r16', n_new=25, seed=9):
    """New users for a warm start against the model of `model_case(name)`: their known feedback (values 1 among them: the
    default confidence log2(1) = 0, not folded in but still seen) and one held-out item each."""
    case = model_case(name)
    rng = np.random.RandomState(seed)
    n_items = case['n_items']
    tu, ti, tf, hu, hi = [], [], [], [], []
    for u in range(n_new):
        items = rng.permutation(n_items)[:rng.randint(3, 12)]
        vals = rng.randint(1, 6, size=len(items)).astype(np.float64)
        vals[0] = 1.0                                   # at least one confidence-0 entry per user
        hu.append(u), hi.append(items[-1])
        order = np.argsort(items[:-1])
        tu += [u] * (len(items) - 1)
        ti += list(items[:-1][order])
        tf += list(vals[:-1][order])
    return dict(case=case, test=(np.array(tu, dtype=np.int64), np.array(ti, dtype=np.int64), np.array(tf)),
                holdout=(np.array(hu, dtype=np.int64), np.array(hi, dtype=np.int64), np.ones(n_new)), n_new=n_new)


def warm_data(w):
    from polara_amd.data import ArrayData
    case = w['case']
    base = model_data(*case['triplets'], case['n_users'], case['n_items'], case['seed'])
    return ArrayData(tuple(base.training), n_users=case['n_users'], n_items=case['n_items'], test=w['test'], holdout=w['holdout'],
                     warm_start=True, fields=('userid', 'itemid', 'rating'))
