"""NumPy restatement of EASE (Steck 2019) for the tests of polara_amd.ease: the weights through `np.linalg.inv` of the
dense X^T X + lambda I, the scores, and the seeded fixtures the host and the GPU tests share.  Lists are selected and
compared with tests/i2i_reference.py (`select`, `classes`, `tie_aware_mismatches`): the total order is the same."""
import numpy as np
import scipy.sparse as sps

# (users, items, about this many entries per user): the three fixtures of the weights and the model tests
FIXTURES = {'small': (300, 120, 12), 'medium': (1000, 257, 20), 'large': (3000, 1000, 30)}
LAMBDAS = (0.5, 10.0, 500.0)


def gram(A, lam):
    """Dense K = A^T A + lam I of a SciPy sparse A (entries exact for integer and half-integer feedback)."""
    G = np.asarray((A.T @ A).todense(), dtype=np.float64)
    return G + float(lam) * np.eye(G.shape[0])


def ease_weights(A, lam):
    """B = I - P diag(1 / diag P) with P = (A^T A + lam I)^-1 and the diagonal set to exactly 0.  Returns (B, P)."""
    P = np.linalg.inv(gram(A, lam))
    B = -P / np.diag(P)[None, :]
    np.fill_diagonal(B, 0.0)
    return B, P


def ease_scores(B, T):
    """Dense scores of the rows of the SciPy sparse test matrix T."""
    return np.asarray(T @ B)


def precision_from_weights(B, d):
    """P rebuilt from the device's outputs: P_ij = -B_ij d_j off the diagonal, P_jj = d_j."""
    P = -np.asarray(B, dtype=np.float64) * np.asarray(d, dtype=np.float64)[None, :]
    P[np.diag_indices_from(P)] = d
    return P


def inverse_residual(P, K):
    """max |P K - I|"""
    return float(np.abs(P @ K - np.eye(K.shape[0])).max())


def training(name, half_steps=False):
    """(idx [nnz x 2], val, shape) of a seeded fixture: every user draws 1 .. 2 * per - 1 distinct items (about `per` on
    average), feedback 1..5 (or 0.5 .. 5 in half steps), and every item has at least one entry."""
    n_users, n_items, per = FIXTURES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 2 * int(half_steps))
    us, its = [], []
    for u in range(n_users):
        k = min(n_items, int(rng.integers(1, 2 * per)))
        its.append(rng.choice(n_items, k, replace=False))
        us.append(np.full(k, u))
    us, its = np.concatenate(us), np.concatenate(its)
    missing = np.setdiff1d(np.arange(n_items), its)
    us = np.r_[us, rng.integers(0, n_users, len(missing))]
    its = np.r_[its, missing]
    pairs = np.unique(np.stack([us, its], 1), axis=0)
    val = rng.integers(1, 11 if half_steps else 6, len(pairs)) * (0.5 if half_steps else 1.0)
    return pairs.astype(np.int64), val.astype(np.float64), (n_users, n_items)


def training_matrix(idx, val, shape, implicit=False):
    A = sps.csr_matrix((np.asarray(val, dtype=np.float64), (idx[:, 0], idx[:, 1])), shape=tuple(shape))
    if implicit:
        A.data = np.sign(A.data)
    return A


def test_rows(name, n_test=40):
    """(users, items, feedback) of `n_test` test rows over a fixture's catalogue in the style of the item-to-item tests:
    the rows 1, 8, 15, ... hold only zero-feedback entries, row 2 is a heavy user (60 % of the catalogue) and the last three
    rows are empty (the model numbers its test users without gaps, so empty rows can only trail).  Every row appears in
    the returned holdout, so the test matrix has n_test rows."""
    _, n_items, per = FIXTURES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 77)
    tu, ti, tv = [], [], []
    for r in range(n_test - 3):
        kind = r % 7
        k = int(0.6 * n_items) if r == 2 else min(n_items, int(rng.integers(1, per + 1)))
        items = np.sort(rng.choice(n_items, k, replace=False))
        vals = np.zeros(k) if kind == 1 else rng.integers(1, 6, k).astype(np.float64)
        tu.append(np.full(k, r))
        ti.append(items)
        tv.append(vals)
    test = tuple(np.concatenate(x) for x in (tu, ti, tv))
    holdout = (np.arange(n_test), rng.integers(0, n_items, n_test), np.ones(n_test))
    return (test[0].astype(np.int64), test[1].astype(np.int64), test[2].astype(np.float64)), holdout, (n_test, n_items)
