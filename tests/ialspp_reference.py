"""TEST-ONLY NumPy restatement of iALS++ (polara_amd/ialspp.py, csrc/ialspp.hip) on top of tests/ials_reference.py: the cached
predictions, the block step as a per-row loop with H and g formed in storage order, the half-sweep, the fit, the objective
with a regularisation per row, the error bounds of a block step, and the CPU double of the iALS++ operators.  Never imported by
the package."""
import numpy as np
import scipy.sparse as sps
import torch

import ials_reference as ials_ref
from ials_reference import EPS, NotPositiveDefinite, as_csr, chol_solve, lapack_solve
from polara_amd import ials, ialspp

MAX_RANK = 2048
BLOCK_SIZES = (16, 32, 64)


def _lam(lam, u):
    return float(lam[u]) if np.ndim(lam) else float(lam)


def row_regularization(C, regularization, exponent=0.0, unobserved=1.0):
    """regularization * (n_row + unobserved * n_other_side) ** exponent per row of C; the float itself when the exponent is 0"""
    indptr, _, _, shape = as_csr(C)
    if float(exponent) == 0.0:
        return float(regularization)
    return float(regularization) * (np.diff(indptr).astype(np.float64) + float(unobserved) * float(shape[1])) ** float(exponent)


def predict(C, X, Y):
    """e[p] = x_u . y_i for every stored entry, storage order"""
    indptr, indices, _, shape = as_csr(C)
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    return np.einsum('ij,ij->i', X[rows], Y[indices])


def block_system(idx, c, e, Ypi, Gpp, r, lam, xpi, skip=None):
    """(H, g) of one row and one block, the sums in storage order; skip: position of an interaction to leave out"""
    H = Gpp + lam * np.eye(len(xpi))
    g = r + lam * xpi
    for p, (i, ci, ei) in enumerate(zip(idx, c, e)):
        if p == skip:
            continue
        y = Ypi[i]
        H = H + (ci - 1.0) * np.outer(y, y)
        g = g + ((ci - 1.0) * ei - ci) * y
    return H, g


def block_step(C, Y, X, E, G, p0, d, lam, R=None, solve=chol_solve, skip_last=False):
    """One block step in place on X and E (float64 arrays; E in storage order) over pi = [p0, min(p0 + d, k)).  lam: a float or
    one value per row.  R = X G[:, pi] of the X the step starts from (formed here when None).  An empty row gets x_pi = 0.
    Raises NotPositiveDefinite with (count, first row) when `solve` refuses rows; those rows are left as they were.
    skip_last: leave the last interaction of every row out of H and g (what a kernel that loses one term computes)."""
    indptr, indices, data, shape = as_csr(C)
    k = Y.shape[1]
    p1 = min(p0 + d, k)
    Ypi = Y[:, p0:p1]
    Gpp = G[p0:p1, p0:p1]
    R = X @ G[:, p0:p1] if R is None else R
    bad = []
    for u in range(shape[0]):
        lo, hi = indptr[u], indptr[u + 1]
        if hi == lo:
            X[u, p0:p1] = 0.0
            continue
        H, g = block_system(indices[lo:hi], data[lo:hi], E[lo:hi], Ypi, Gpp, R[u], _lam(lam, u), X[u, p0:p1],
                            skip=hi - lo - 1 if skip_last else None)
        try:
            delta = solve(H, g)
        except NotPositiveDefinite:
            bad.append(u)
            continue
        X[u, p0:p1] -= delta
        E[lo:hi] -= Ypi[indices[lo:hi]] @ delta
    if bad:
        err = NotPositiveDefinite('iALS++ block step: %d row(s) whose block system is not positive definite, the first is row %d'
                                  % (len(bad), bad[0]))
        err.count, err.first = len(bad), bad[0]
        raise err
    return X, E


def half_sweep(C, Y, X, G, lam, d, solve=chol_solve, after_block=None):
    """predict, then the blocks in ascending order, in place on X; returns (X, E).  after_block(p0, X, E) is called after each."""
    E = predict(C, X, Y)
    for p0 in range(0, Y.shape[1], d):
        block_step(C, Y, X, E, G, p0, d, lam, solve=solve)
        if after_block is not None:
            after_block(p0, X, E)
    return X, E


def objective_terms(C, X, Y, lam_rows, lam_cols):
    """(the objective sum over all pairs of w (p - x.y)^2 + sum_u lam_rows[u] |x_u|^2 + sum_i lam_cols[i] |y_i|^2 computed
    densely, the sum of the absolute values of its terms, their number)"""
    indptr, indices, data, shape = as_csr(C)
    S = X @ Y.T
    W = np.ones(shape)
    P = np.zeros(shape)
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    W[rows, indices] = data
    P[rows, indices] = 1.0
    fit_terms = W * (P - S) ** 2
    reg_terms = np.concatenate(((np.asarray(lam_rows) * (X * X).T).ravel(), (np.asarray(lam_cols) * (Y * Y).T).ravel()))
    total = float(fit_terms.sum() + reg_terms.sum())
    return total, float(np.abs(fit_terms).sum() + np.abs(reg_terms).sum()), fit_terms.size + reg_terms.size


def objective(C, X, Y, lam_rows, lam_cols):
    return objective_terms(C, X, Y, lam_rows, lam_cols)[0]


def objective_by_traces(C, X, Y, lam_rows, lam_cols):
    """the same by  tr(X^T X Y^T Y) + sum_nz [c (1 - s)^2 - s^2] + the regularisation"""
    indptr, indices, data, shape = as_csr(C)
    s = predict(C, X, Y)
    GX, GY = X.T @ X, Y.T @ Y
    reg = (np.asarray(lam_rows) * (X * X).sum(axis=1)).sum() + (np.asarray(lam_cols) * (Y * Y).sum(axis=1)).sum()
    return float((GX * GY).sum() + (data * (1.0 - s) ** 2 - s * s).sum() + reg)


def fit(C, rank, lam, num_epochs, d, seed=None, init=None, solve=chol_solve, loss_history=None, reg_exponent=0.0, reg_unobserved=1.0):
    """(X, Y) after `num_epochs` times (user half-sweep, item half-sweep) from `ials.initial_factors`"""
    C = sps.csr_matrix(C.m if hasattr(C, 'm') else C)
    Ct = sps.csr_matrix(C.T)
    Ct.sort_indices()
    X0, Y0 = ials.initial_factors(C.shape[0], C.shape[1], rank, seed) if init is None else init
    X, Y = np.array(X0, dtype=np.float64), np.array(Y0, dtype=np.float64)
    lu, li = (row_regularization(M, lam, reg_exponent, reg_unobserved) for M in (C, Ct))
    for _ in range(int(num_epochs)):
        half_sweep(C, Y, X, Y.T @ Y, lu, d, solve)
        if loss_history is not None:
            loss_history.append(objective_by_traces(C, X, Y, lu, li))
        half_sweep(Ct, X, Y, X.T @ X, li, d, solve)
        if loss_history is not None:
            loss_history.append(objective_by_traces(C, X, Y, lu, li))
    return X, Y


def step_bounds(C, Y, G, lam, X0, E0, p0, d, X1, R=None):
    """Per row of C the bound on |x^_pi - x_pi|_2 of a backward-stable block step in fp64 against the reference step X0 -> X1
    (E0 the predictions the step starts from): `ials_reference.row_bounds` for the block system — H, g, the block width dw in
    place of A, b, k —
        4 kappa_2(H) eps [ (n + 2) S_H / |H|_2 + dw (3 dw + 1) + (n + 2) S_g / |g|_2 ] (|x0_pi|_2 + |x1_pi|_2),
    S_H = |G[pi,pi]|_2 + lam + sum |c - 1| |y_pi|^2,  S_g = |r| + lam |x0_pi| + sum (|c - 1| |e| + c) |y_pi| (g has n + 2 terms, and
    the coefficient of an entry is itself rounded).  |x_u| of the half-step's bound becomes |x0_pi| + |x1_pi| because the step
    solves for their difference: |delta| <= |x0_pi| + |x1_pi|.  0 for an empty row.
    Also returns per stored entry the bound on |e^ - e| after the step: n d eps (|e0| + sum_j |y_ij| |delta_j|), n the entries
    of the row, d the block size (0 for a row that the step leaves alone)."""
    indptr, indices, data, shape = as_csr(C)
    k = Y.shape[1]
    p1 = min(p0 + d, k)
    dw = p1 - p0
    Ypi, Gpp = Y[:, p0:p1], G[p0:p1, p0:p1]
    R = X0 @ G[:, p0:p1] if R is None else R
    g2 = np.linalg.norm(Gpp, 2)
    ynorm = np.linalg.norm(Ypi, axis=1)
    rows, entries = np.zeros(shape[0]), np.zeros(len(indices))
    for u in range(shape[0]):
        lo, hi = indptr[u], indptr[u + 1]
        n = hi - lo
        if n == 0:
            continue
        idx, c, e = indices[lo:hi], data[lo:hi], E0[lo:hi]
        lam_u = _lam(lam, u)
        H, g = block_system(idx, c, e, Ypi, Gpp, R[u], lam_u, X0[u, p0:p1])
        sv = np.linalg.svd(H, compute_uv=False)
        S_H = g2 + lam_u + (np.abs(c - 1.0) * ynorm[idx] ** 2).sum()
        S_g = np.linalg.norm(R[u]) + lam_u * np.linalg.norm(X0[u, p0:p1]) + ((np.abs(c - 1.0) * np.abs(e) + c) * ynorm[idx]).sum()
        with np.errstate(divide='ignore'):
            bracket = (n + 2) * S_H / sv[0] + dw * (3 * dw + 1) + (n + 2) * S_g / np.linalg.norm(g)
        rows[u] = 4.0 * (sv[0] / sv[-1]) * EPS * bracket * (np.linalg.norm(X0[u, p0:p1]) + np.linalg.norm(X1[u, p0:p1]))
        delta = X0[u, p0:p1] - X1[u, p0:p1]
        entries[lo:hi] = n * d * EPS * (np.abs(e) + np.abs(Ypi[idx]) @ np.abs(delta))
    return rows, entries


def dropped_interaction_margin(C, Y, G, lam, X0, E0, p0, d, X1, bounds, R=None):
    """the smallest over the rows with more than one entry of |x_pi(last interaction dropped) - x_pi| / bound: how far
    outside the tolerance a kernel that loses a single term of H and g lands"""
    indptr = as_csr(C)[0]
    Xd, Ed = X0.copy(), E0.copy()
    block_step(C, Y, Xd, Ed, G, p0, d, lam, R=R, solve=lapack_solve, skip_last=True)
    p1 = min(p0 + d, Y.shape[1])
    many = np.diff(indptr) > 1
    return (np.linalg.norm(Xd[many, p0:p1] - X1[many, p0:p1], axis=1) / bounds[many]).min()


# ---- the CPU double of the iALS++ operators ----------------------------------------------------------------------------------
class IALSPPNumpyOps(ials_ref.IALSNumpyOps):
    """IALSNumpyOps plus what polara_amd/ialspp.py asks of HipOps (same semantics on CPU tensors, in place)."""

    def ialspp_max_rank(self):
        return MAX_RANK

    def ialspp_block_sizes(self):
        return BLOCK_SIZES

    @staticmethod
    def _reg(regularization):
        return regularization.numpy() if isinstance(regularization, torch.Tensor) else float(regularization)

    def ialspp_predict(self, Cm, X, Y, out=None):
        E = torch.from_numpy(predict(Cm, X.numpy(), Y.numpy()))
        if out is not None:
            out.copy_(E)
            return out
        return E

    def ialspp_block_step(self, Cm, Y, X, E, G, p0, block_size, regularization, R=None, row_order=None):
        k = int(Y.shape[1])
        if k < 1 or k > MAX_RANK:
            raise ValueError('iALS++: rank %d outside 1..%d' % (k, MAX_RANK))
        if block_size not in BLOCK_SIZES:
            raise ValueError('iALS++ block step: block size %d is not one of %s' % (block_size, BLOCK_SIZES))
        try:
            block_step(Cm, Y.numpy(), X.numpy(), E.numpy(), G.numpy(), int(p0), int(block_size), self._reg(regularization),
                       R=None if R is None else R.numpy(), solve=self.solve)
        except NotPositiveDefinite as err:
            raise ValueError(str(err) + ' (their factors are left unchanged)')
        return X

    def ialspp_half_sweep(self, Cm, Y, X, G, regularization, block_size, E=None):
        E = self.ialspp_predict(Cm, X, Y, out=E)
        for p0 in range(0, int(Y.shape[1]), int(block_size)):
            self.ialspp_block_step(Cm, Y, X, E, G, p0, block_size, regularization)
        return X, E

    def ialspp_loss(self, Cm, X, Y, reg_rows, reg_cols, GX=None, GY=None):
        return objective_by_traces(Cm, X.numpy(), Y.numpy(), self._reg(reg_rows), self._reg(reg_cols))


# ---- the inputs of the step tests -----------------------------------------------------------------------------------------------
STEP_CASES = [(1, 16, 0), (5, 16, 0), (16, 16, 0), (17, 16, 16), (33, 32, 32), (64, 64, 0), (65, 64, 64), (100, 64, 64), (160, 32, 128),
              (272, 64, 256)]                   # (rank, block size, block start) on confidence_matrix('wide')
DROPPED_MARGIN = 2e7                            # a decade below the smallest margin measured in tests/test_ialspp_host.py (2.2e8)


def start(C, rank, seed=3):
    """X0 = 0.1 randn: the factors a step test starts from"""
    return 0.1 * np.random.RandomState(seed).randn(C.shape[0], rank)


# ---- the inputs of the model tests -------------------------------------------------------------------------------------------
LAMBDA = ials_ref.LAMBDA
TOPK = ials_ref.TOPK
MIN_GAP = 1e-7
EPOCHS = 3
MODEL_CASES = {                     # name: (n_users, n_items, rank, block size, density, seed)
    'r16': (60, 45, 16, 16, 0.15, 2),
    'r40': (50, 40, 40, 16, 0.12, 3),
    'r160': (300, 120, 160, 64, 0.08, 4),
    'r272': (120, 90, 272, 64, 0.1, 5),
}
_cases = {}


def model_case(name):
    """The seeded input of one model test and its restatements, computed once and never written to — the construction of
    `ials_reference.model_case` with the iALS++ fit: `X`, `Y`, `loss` the Cholesky statement's factors and objective per
    half-sweep, `d` the largest relative distance of its factors to those of the statement with np.linalg.solve, `lists` /
    `gaps` the top lists of the test users and the smallest adjacent gap among their top TOPK + 1 scores."""
    if name in _cases:
        return _cases[name]
    n_users, n_items, rank, block, density, seed = MODEL_CASES[name]
    u, i, r = ials_ref.ratings_matrix(seed, n_users, n_items, density)
    f = r ** np.array([0.5, 1.0, 3.0])[np.random.RandomState(seed + 100).randint(3, size=len(r))]
    data = ials_ref.model_data(u, i, f, n_users, n_items, seed)
    tu, ti, tf = data.training
    C = sps.csr_matrix((np.log2(tf), (tu, ti)), shape=(n_users, n_items))
    C.sort_indices()
    loss = []
    X, Y = fit(C, rank, LAMBDA, EPOCHS, block, seed=seed, loss_history=loss)
    X2, Y2 = fit(C, rank, LAMBDA, EPOCHS, block, seed=seed, solve=lapack_solve)
    d = max(ials_ref.rel_distance(X2, X), ials_ref.rel_distance(Y2, Y))
    test_users = np.unique(data.test.holdout.userid)
    sel = np.isin(tu, test_users)
    lists, gaps = ials_ref.lists_and_gaps(X[test_users] @ Y.T, (np.searchsorted(test_users, tu[sel]), ti[sel]))
    case = dict(name=name, n_users=n_users, n_items=n_items, rank=rank, block=block, epochs=EPOCHS, seed=seed, triplets=(u, i, f), C=C,
                X=X, Y=Y, loss=np.array(loss), d=d, test_users=test_users, lists=lists, gaps=gaps)
    for a in (X, Y, lists, gaps):
        a.setflags(write=False)
    _cases[name] = case
    return case


def model_for(case, ops, data=None, **kwargs):
    m = ials_ref.model_for(case, ops, cls=ialspp.ImplicitALSPP, data=data, **kwargs)
    m.block_size = case['block']
    return m


def warm_case(name='r16', n_new=25, seed=9):
    """`ials_reference.warm_case` against the iALS++ model of `model_case(name)`"""
    w = ials_ref.warm_case('r16', n_new, seed)          # the new users depend on the item count alone
    assert ials_ref.MODEL_CASES['r16'][1] == MODEL_CASES[name][1]
    return dict(w, case=model_case(name))


def fold_in(Cw, Y, G, lam, d, sweeps, solve=chol_solve):
    """the warm-start users' factors: `sweeps` user half-sweeps from zero"""
    X = np.zeros((Cw.shape[0], Y.shape[1]))
    for _ in range(sweeps):
        half_sweep(Cw, Y, X, G, lam, d, solve)
    return X
