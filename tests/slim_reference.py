"""NumPy restatement of the SLIM solver's contract (include/polara_hip.h, csrc/slim.hip) for the tests of polara_amd.slim:
the plain loop exactly as the header states it, a vectorised "screened" form of it (all coordinates of a chunk are
evaluated at once, the lowest changing one is applied: the same bits, much faster), the dense scores in SciPy's order and
the objective.  Python floats and NumPy fp64 round every product, sum and quotient on its own, as the contract demands.
Fixtures and test rows are those of tests/ease_reference.py; lists are selected and compared with tests/i2i_reference.py."""
import math

import numpy as np
import scipy.sparse as sps

import ease_reference as ease_ref
import sim_reference as sim_ref

FIXTURES = ease_ref.FIXTURES
training, training_matrix, test_rows = ease_ref.training, ease_ref.training_matrix, ease_ref.test_rows
PENALTIES = ((0.0, 10.0), (1.0, 5.0), (5.0, 0.5), (20.0, 50.0))           # (l1, l2) of the fixture tests
CHUNK = 128                                                              # coordinates the screened form evaluates at once


def gram(A):
    """Dense G = A^T A of a SciPy sparse A, with its diagonal (entries exact for integer feedback)."""
    return np.ascontiguousarray(np.asarray((A.T @ A).todense(), dtype=np.float64))


def sized_training(n):
    """Seeded integer-valued X with n items: 3 n users (at least 8) of up to 10 items each, every item present (the
    inputs of the tile-edge tests, in the style of the EASE ones)."""
    rng = np.random.default_rng(7000 + n)
    n_users, per = max(8, 3 * n), min(n, 10)
    us, its = [], []
    for u in range(n_users):
        k = int(rng.integers(1, per + 1))
        its.append(rng.choice(n, k, replace=False))
        us.append(np.full(k, u))
    us, its = np.concatenate(us), np.concatenate(its)
    missing = np.setdiff1d(np.arange(n), its)
    pairs = np.unique(np.stack([np.r_[us, rng.integers(0, n_users, len(missing))], np.r_[its, missing]], 1), axis=0)
    return pairs.astype(np.int64), rng.integers(1, 6, len(pairs)).astype(np.float64), (n_users, n)


def solve_column_plain(G, j, l1, l2, tol, max_sweeps, positive=True):
    """(w, sweeps) of target column j: the contract's loop, statement by statement."""
    n = G.shape[0]
    l1, l2, tol = float(l1), float(l2), float(tol)
    w = np.zeros(n)
    r = G[j].astype(np.float64).copy()
    sweep = 0
    while sweep < max_sweeps:
        sweep += 1
        dmax = wmax = 0.0
        for k in range(n):
            if k == j:
                continue
            gkk = float(G[k, k])
            den = gkk + l2
            if not den > 0:
                continue
            old = float(w[k])
            rho = float(r[k]) + gkk * old
            if positive:
                t = rho - l1
                new = t / den if t > 0 else 0.0
            else:
                t = abs(rho) - l1
                new = math.copysign(t / den, rho) if t > 0 else 0.0
            d = new - old
            if d != 0:
                r = r - d * G[k]
                w[k] = new
            dmax = max(dmax, abs(d))
            wmax = max(wmax, abs(new))
        if wmax == 0 or dmax <= tol * wmax:
            break
    return w, sweep


def solve_column(G, j, l1, l2, tol, max_sweeps, positive=True, diag=None):
    """(w, sweeps) of target column j in the screened form: between two changes r is constant, so a chunk of coordinates
    is evaluated at once, the lowest one that changes is applied and the evaluation continues behind it."""
    n = G.shape[0]
    l1, l2, tol = float(l1), float(l2), float(tol)
    diag = np.ascontiguousarray(np.diagonal(G)) if diag is None else diag
    den_all = diag + l2
    ok_all = den_all > 0
    ok_all[j] = False
    safe_den = np.where(ok_all, den_all, 1.0)
    w = np.zeros(n)
    r = G[j].astype(np.float64).copy()
    sweep = 0
    while sweep < max_sweeps:
        sweep += 1
        dmax = wmax = 0.0
        k0 = 0
        while k0 < n:
            hi = min(n, k0 + CHUNK)
            ok = ok_all[k0:hi]
            old = w[k0:hi]
            rho = r[k0:hi] + diag[k0:hi] * old
            if positive:
                t = rho - l1
                new = np.where(t > 0, t / safe_den[k0:hi], 0.0)
            else:
                t = np.abs(rho) - l1
                new = np.where(t > 0, np.copysign(t / safe_den[k0:hi], rho), 0.0)
            d = np.where(ok, new - old, 0.0)
            changed = np.flatnonzero(d != 0)
            stop = hi - k0 if len(changed) == 0 else int(changed[0]) + 1
            done = np.abs(new[:stop])[ok[:stop]]
            if len(done):
                wmax = max(wmax, float(done.max()))
            if len(changed) == 0:
                k0 = hi
                continue
            c = stop - 1
            dmax = max(dmax, abs(float(d[c])))
            r = r - d[c] * G[k0 + c]
            w[k0 + c] = new[c]
            k0 += stop
        if wmax == 0 or dmax <= tol * wmax:
            break
    return w, sweep


def solve_columns(G, columns, l1, l2, tol=1e-4, max_sweeps=100, positive=True, plain=False):
    """(Wt [len(columns) x n]: row c is w of target column columns[c], sweeps int32) of the listed target columns."""
    columns = list(columns)
    G = np.ascontiguousarray(G, dtype=np.float64)
    diag = np.ascontiguousarray(np.diagonal(G))
    Wt = np.zeros((len(columns), G.shape[0]))
    sweeps = np.zeros(len(columns), dtype=np.int32)
    for c, j in enumerate(columns):
        if plain:
            Wt[c], sweeps[c] = solve_column_plain(G, j, l1, l2, tol, max_sweeps, positive)
        else:
            Wt[c], sweeps[c] = solve_column(G, j, l1, l2, tol, max_sweeps, positive, diag)
    return Wt, sweeps


def slim_weights(G, l1, l2, tol=1e-4, max_sweeps=100, positive=True):
    """(W [n x n] with W[i, j] the weight of source item i for target j, sweeps) over all columns."""
    Wt, sweeps = solve_columns(G, range(G.shape[0]), l1, l2, tol, max_sweeps, positive)
    return np.ascontiguousarray(Wt.T), sweeps


def slim_scores(W, T):
    """Dense scores T W of the rows of the SciPy sparse test matrix T, summed in the order of SciPy's sparse product (the
    order of the device's scoring pass)."""
    return sim_ref.product(T, sps.csr_matrix(W))


def objective(X, j, w, l1, l2):
    """1/2 |x_j - X w|^2 + l1 |w|_1 + l2 / 2 |w|^2 for the SciPy sparse or dense X."""
    X = np.asarray(X.todense()) if sps.issparse(X) else np.asarray(X)
    res = X[:, j] - X @ w
    return 0.5 * float(res @ res) + l1 * float(np.abs(w).sum()) + 0.5 * l2 * float(w @ w)
