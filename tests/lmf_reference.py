"""TEST-ONLY NumPy restatement of logistic matrix factorisation (polara_amd/lmf.py, csrc/lmf.hip; the specification is the comment
in include/polara_hip.h): the draw stream, the half-step row by row in the order of the specification, the fit, an independent
np.longdouble evaluation in plain order with its first-order error bound, the CPU double of the LMF operators on top of
tests/numpy_ops.py, and the small fixtures.  Never imported by the package."""
import numpy as np
import scipy.sparse as sps
import torch

from bpr_reference import MASK, mix64, sigmoid, stream_key
from ials_reference import (CONFIDENCES, IALSNumpyOps, as_csr, check_lists, item_block, lists_and_gaps, model_data,  # noqa: F401
                            ratings_matrix, rel_distance)
from polara_amd import lmf

MAX_RANK = 126
CHAINS = 4                          # PK_LMF_CHAINS of include/polara_hip.h
EPS = 2.0 ** -53
SIGMOID_MAX_REL_ERR = 2.98e-16      # of the restated sigmoid against np.longdouble: measured in test_bpr_host.py
FOLD_IN_ROUND = 0x80000000


# ---- the draws ---------------------------------------------------------------------------------------------------------------
def neg_pointers(indptr, n_other, neg_prop):
    """int64 [n_rows + 1]: the exclusive prefix sum of m = min(n_other, n * neg_prop) over the rows"""
    m = np.minimum(np.diff(np.asarray(indptr, dtype=np.int64)) * int(neg_prop), int(n_other))
    return np.concatenate(([0], np.cumsum(m))).astype(np.int64)


def _mix64_array(z):
    """the splitmix64 output function on a uint64 array (arithmetic modulo 2**64)"""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draws(key, start, m, n_other):
    """int64 [m]: negatives t = 0 .. m - 1 of the row whose counter starts at `start` = neg_ptr[u]"""
    with np.errstate(over='ignore'):
        counter = np.uint64(int(key)) + np.uint64(int(start)) + np.arange(int(m), dtype=np.uint64)
        w = _mix64_array(counter) >> np.uint64(32)
    return ((w * np.uint64(int(n_other))) >> np.uint64(32)).astype(np.int64)


def naive_draws(key, start, m, n_other):
    """the same, sample by sample on Python integers"""
    return np.array([((mix64((int(key) + int(start) + t) & MASK) >> 32) * int(n_other)) >> 32 for t in range(int(m))], dtype=np.int64)


def draw_negatives(C, neg_prop, seed, rnd):
    """int32 [neg_ptr[-1]]: what HipOps.lmf_draw_negatives returns for the matrix C"""
    indptr, _, _, shape = as_csr(C)
    ptr = neg_pointers(indptr, shape[1], neg_prop)
    key = stream_key(seed, rnd)
    parts = [draws(key, ptr[u], ptr[u + 1] - ptr[u], shape[1]) for u in range(shape[0])]
    return np.concatenate(parts + [np.zeros(0, dtype=np.int64)]).astype(np.int32)


# ---- the half-step -----------------------------------------------------------------------------------------------------------
def row_samples(indices, conf, key, start, n_other, neg_prop):
    """(columns of the sample list — positives in storage order, then negatives in draw order —, n)"""
    n = len(indices)
    m = min(int(n_other), n * int(neg_prop))
    return np.concatenate([np.asarray(indices, dtype=np.int64), draws(key, start, m, n_other)]), n


def serial_sum(P):
    """the rows of P added left to right onto zeros: np.cumsum is strictly sequential along its axis"""
    return np.cumsum(np.vstack([np.zeros((1, P.shape[1])), P]), axis=0)[-1]


def row_step(x, a, cols, n, conf, Y, lr, reg, pinned, chains=CHAINS):
    """(x_new, a_new) of one row from its sample list, in the order of the specification"""
    K = len(x)
    Yg = Y[cols]
    with np.errstate(all='ignore'):
        s = x[0] * Yg[:, 0]
        for c in range(1, K):
            s = s + x[c] * Yg[:, c]
        g = np.empty(len(cols))
        g[:n] = conf * sigmoid(s[:n])
        g[n:] = -sigmoid(-s[n:])
        P = g[:, None] * Yg
        D = serial_sum(P[0::chains])
        for j in range(1, chains):
            D = D + serial_sum(P[j::chains])
        d = D - reg * x
        a_new = a + d * d
        x_new = x + (lr / np.sqrt(1e-6 + a_new)) * d
    if pinned >= 0:
        x_new[pinned], a_new[pinned] = x[pinned], a[pinned]
    return x_new, a_new


def plain_row_step(x, a, cols, n, conf, Y, lr, reg, pinned):
    """the same with one chain, as a plain Python loop over samples and columns on NumPy doubles"""
    K = len(x)
    D = [np.float64(0.0)] * K
    with np.errstate(all='ignore'):
        for q, i in enumerate(cols):
            y = Y[i]
            s = x[0] * y[0]
            for c in range(1, K):
                s = s + x[c] * y[c]
            g = conf[q] * sigmoid(s) if q < n else -sigmoid(-s)
            for c in range(K):
                D[c] = D[c] + g * y[c]
        x_new, a_new = x.copy(), a.copy()
        for c in range(K):
            if c == pinned:
                continue
            d = D[c] - reg * x[c]
            a_new[c] = a[c] + d * d
            x_new[c] = x[c] + (lr / np.sqrt(1e-6 + a_new[c])) * d
    return x_new, a_new


def half_step(C, Y, X, A, lr, reg, neg_prop, seed, rnd, pinned, chains=CHAINS, step=row_step, drop=None):
    """(X_new, A_new): one half-step over the rows of C against the fixed Y; an empty row is not touched.  drop = 'positive' /
    'negative': the last positive / negative of every row is left out (the lost-term margins of the tests)."""
    indptr, indices, data, shape = as_csr(C)
    ptr = neg_pointers(indptr, shape[1], neg_prop)
    key = stream_key(seed, rnd)
    X, A = np.array(X, dtype=np.float64), np.array(A, dtype=np.float64)
    for u in range(shape[0]):
        lo, hi = indptr[u], indptr[u + 1]
        if hi == lo:
            continue
        cols, n = row_samples(indices[lo:hi], data[lo:hi], key, ptr[u], shape[1], neg_prop)
        conf = data[lo:hi]
        if drop == 'positive':
            cols, conf, n = np.delete(cols, n - 1), conf[:-1], n - 1
        elif drop == 'negative':
            cols = cols[:-1]
        args = (X[u].copy(), A[u].copy(), cols, n, conf, Y, lr, reg, pinned)
        X[u], A[u] = step(*args, chains) if step is row_step else step(*args)
    return X, A


def half_step_longdouble(C, Y, X, A, lr, reg, neg_prop, seed, rnd, pinned):
    """(X_new, A_new) as np.longdouble arrays: an independent evaluation in plain order — NumPy's own dot products, sums and exp
    in extended precision, no chains, no restated sigmoid; and (BX, BA), the first-order bounds of `half_step_bounds`."""
    L = np.longdouble
    indptr, indices, data, shape = as_csr(C)
    ptr = neg_pointers(indptr, shape[1], neg_prop)
    key = stream_key(seed, rnd)
    Xn, An = np.array(X, dtype=L), np.array(A, dtype=L)
    BX, BA = np.zeros(X.shape), np.zeros(A.shape)
    Yl = np.asarray(Y, dtype=L)
    for u in range(shape[0]):
        lo, hi = indptr[u], indptr[u + 1]
        if hi == lo:
            continue
        cols, n = row_samples(indices[lo:hi], data[lo:hi], key, ptr[u], shape[1], neg_prop)
        x, a, Yg = Xn[u].copy(), An[u].copy(), Yl[cols]
        s = Yg @ x
        g = np.concatenate([data[lo:hi].astype(L) / (1 + np.exp(s[:n])), -1 / (1 + np.exp(-s[n:]))])
        D = g @ Yg
        d = D - L(reg) * x
        a_new = a + d * d
        h = L(lr) / np.sqrt(L(1e-6) + a_new)
        x_new = x + h * d
        BX[u], BA[u] = (np.asarray(b, dtype=np.float64) for b in half_step_bounds(x, Yg, s, g, D, d, a, a_new, h, x_new, lr, reg))
        keep = np.arange(len(x)) != pinned
        Xn[u, keep], An[u, keep] = x_new[keep], a_new[keep]
        BX[u, ~keep] = BA[u, ~keep] = 0.0
    return Xn, An, BX, BA


def half_step_bounds(x, Yg, s, g, D, d, a, a_new, h, x_new, lr, reg, chains=CHAINS):
    """First-order bounds on |x^ - x_new| and |a^ - a_new| per column for the fp64 half-step in the order of the specification,
    eps = 2^-53, T samples, K columns, ax = |x|, aY = |Yg|, ag = |g| (the derivation is the docstring of
    test_lmf_host.test_restatement_against_longdouble):
        ds_q = K eps sum_c |x_c y_qc|                               (a serial dot product of K terms)
        rg_q = ds_q + SIGMOID_MAX_REL_ERR + eps                     (|d log sigm / ds| <= 1; the sigmoid's own error; c * sigm)
        dD_c = sum_q |g_q y_qc| (rg_q + (ceil(T / chains) + chains) eps)       (the product, the chain, the chains' sum)
        dd_c = dD_c + eps (|reg x_c| + |d_c|)
        da_c = 2 |d_c| dd_c + eps (d_c^2 + a_new_c)
        dh_c = h_c (da_c / (2 (1e-6 + a_new_c)) + 3 eps)            (the sum under the root, the root, the division)
        dx_c = h_c dd_c + |d_c| dh_c + eps (|h_c d_c| + |x_new_c|)
    each doubled: the slack for the second-order terms and for the longdouble evaluation's own error."""
    f = lambda v: np.abs(np.asarray(v, dtype=np.float64))
    T, K = Yg.shape
    ax, aY, ag = f(x), f(Yg), f(g)
    ds = K * EPS * (aY @ ax)
    rg = ds + SIGMOID_MAX_REL_ERR + EPS
    depth = -(-T // chains) + chains
    dD = (ag * (rg + depth * EPS)) @ aY
    dd = dD + EPS * (abs(reg) * ax + f(d))
    da = 2 * f(d) * dd + EPS * (f(d) ** 2 + f(a_new))
    dh = f(h) * (da / (2 * (1e-6 + f(a_new))) + 3 * EPS)
    dx = f(h) * dd + f(d) * dh + EPS * (f(h) * f(d) + f(x_new))
    return 2 * dx, 2 * da


def fit(C, rank, lr, reg, neg_prop, num_epochs, seed, init=None, chains=CHAINS):
    """(X, Y) after `num_epochs` times (user half-step, item half-step) from `lmf.initial_factors`"""
    C = sps.csr_matrix(C.m if hasattr(C, 'm') else C)
    Ct = sps.csr_matrix(C.T)
    Ct.sort_indices()
    X0, Y0 = lmf.initial_factors(C.shape[0], C.shape[1], rank, seed) if init is None else init
    X, Y = np.array(X0, dtype=np.float64), np.array(Y0, dtype=np.float64)
    K = rank + 2
    AX, AY = np.zeros_like(X), np.zeros_like(Y)
    for epoch in range(int(num_epochs)):
        X, AX = half_step(C, Y, X, AX, lr, reg, neg_prop, seed, 2 * epoch, K - 1, chains)
        Y, AY = half_step(Ct, X, Y, AY, lr, reg, neg_prop, seed, 2 * epoch + 1, K - 2, chains)
    return X, Y


def fold_in(Cw, Y, lr, reg, neg_prop, seed, epochs):
    """the warm-start rows: `epochs` user half-steps from factors 0, bias 0, pinned 1, state 0, rounds 0x80000000 | t"""
    K = Y.shape[1]
    X, A = np.zeros((Cw.shape[0], K)), np.zeros((Cw.shape[0], K))
    X[:, K - 1] = 1.0
    for t in range(int(epochs)):
        X, A = half_step(Cw, Y, X, A, lr, reg, neg_prop, seed, FOLD_IN_ROUND | t, K - 1)
    return X


# ---- the CPU double of the LMF operators -------------------------------------------------------------------------------------
class LMFNumpyOps(IALSNumpyOps):
    """NumpyOps (with the confidence helpers of the iALS double) plus what polara_amd/lmf.py asks of HipOps"""

    def lmf_max_rank(self):
        return MAX_RANK

    def lmf_plan(self, Cm, neg_prop):
        neg_prop = int(neg_prop)
        if neg_prop < 1:
            raise ValueError('LMF: neg_prop %d < 1' % neg_prop)
        plans = Cm.__dict__.setdefault('_lmf_plans', {})
        if neg_prop not in plans:
            ptr = neg_pointers(Cm.m.indptr, Cm.shape[1], neg_prop)
            plans[neg_prop] = dict(neg_ptr=torch.from_numpy(ptr), negatives=int(ptr[-1]), neg_prop=neg_prop, matrix=Cm,
                                   shape=tuple(int(x) for x in Cm.shape), row_order=None)
        return plans[neg_prop]

    def lmf_half_step(self, plan, Y, X, A, lr, reg, seed, round, pinned, row_order=None):
        K = int(Y.shape[1])
        if K < 3 or K - 2 > MAX_RANK:
            raise ValueError('LMF: rank %d outside 1..%d' % (K - 2, MAX_RANK))
        Xn, An = half_step(plan['matrix'], Y.numpy(), X.numpy(), A.numpy(), float(lr), float(reg), plan['neg_prop'], seed, round, pinned)
        X.copy_(torch.from_numpy(Xn))
        A.copy_(torch.from_numpy(An))
        return X

    def lmf_draw_negatives(self, plan, seed, round):
        return torch.from_numpy(draw_negatives(plan['matrix'], plan['neg_prop'], seed, round))


# ---- the inputs of the half-step tests ---------------------------------------------------------------------------------------
# 0 .. 9: around PK_LMF_CHAINS; 15 .. 17, 31 .. 33, 63 .. 65: the list of n (1 + neg_prop) samples ends, and its positives end, just
# around the staging chunks (64, 32, 16 or 8 samples) for neg_prop 1 and 3; 257: several chunks; 1 000: the cap (3 000 > 1 100)
WIDE_LENGTHS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 1000]


def confidence_matrix(kind):
    """'wide': 40 x 1 100, the row lengths of WIDE_LENGTHS and the rest random <= 20 — with neg_prop = 3 the cap m = n_other binds
    on the 1 000-entry row and nowhere else;  'tall': 3 000 x 16 — more rows than one wave of workgroups."""
    n_rows, n_cols, seed = {'wide': (40, 1100, 21), 'tall': (3000, 16, 22)}[kind]
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


def blocks(n_rows, n_cols, rank, pinned_side, seed=0):
    """(X [n_rows x K], A [n_rows x K] >= 0, Y [n_cols x K], pinned) of a half-step on the 'user' side (X = [f | b | 1], Y =
    [f | 1 | b], pinned K - 1) or the 'item' side (the roles swapped, pinned K - 2): random factors, biases and state"""
    K = rank + 2
    rng = np.random.RandomState(1000 * rank + seed)
    X, Y = rng.normal(scale=0.3, size=(n_rows, K)), rng.normal(scale=0.3, size=(n_cols, K))
    A = rng.rand(n_rows, K) * 2.0
    px, py = (K - 1, K - 2) if pinned_side == 'user' else (K - 2, K - 1)
    X[:, px], Y[:, py] = 1.0, 1.0
    return X, A, Y, px


def planted_matrix(n_users=60, n_items=40, seed=5):
    """two planted blocks: users of group g like items of group g (density 0.5) and nothing else; returns (dense 0/1 of what is
    stored, the users' groups, the items' groups).  Every user keeps unseen items of its own group."""
    rng = np.random.RandomState(seed)
    ug, ig = np.arange(n_users) % 2, np.arange(n_items) % 2
    dense = ((ug[:, None] == ig[None, :]) & (rng.rand(n_users, n_items) < 0.5)).astype(np.float64)
    return dense, ug, ig


# ---- the inputs of the model tests -------------------------------------------------------------------------------------------
TOPK = 10
LEARNING_RATE, REGULARIZATION = 1.0, 0.6
MODEL_CASES = {                     # name: (n_users, n_items, rank, epochs, neg_prop, density, seed)
    'r5': (37, 29, 5, 3, 2, 0.2, 1),
    'r14': (60, 45, 14, 3, 3, 0.15, 2),
    'r30': (80, 50, 30, 2, 3, 0.12, 3),
}
_cases = {}


def model_case(name):
    """The seeded input of one model test and its restated fit, computed once and never written to (feedback as in
    ials_reference.model_case: the default confidence log2(feedback) is > 0); `lists` / `gaps` the top lists of the test users
    (seen items masked) and the smallest adjacent gap among their top TOPK + 1 scores."""
    if name in _cases:
        return _cases[name]
    n_users, n_items, rank, epochs, neg_prop, density, seed = MODEL_CASES[name]
    u, i, r = ratings_matrix(seed, n_users, n_items, density)
    f = r ** np.array([0.5, 1.0, 3.0])[np.random.RandomState(seed + 100).randint(3, size=len(r))]
    data = model_data(u, i, f, n_users, n_items, seed)
    tu, ti, tf = data.training
    C = sps.csr_matrix((np.log2(tf), (tu, ti)), shape=(n_users, n_items))
    C.sort_indices()
    X, Y = fit(C, rank, LEARNING_RATE, REGULARIZATION, neg_prop, epochs, seed)
    test_users = np.unique(data.test.holdout.userid)
    rows = np.isin(tu, test_users)
    lists, gaps = lists_and_gaps(X[test_users] @ Y.T, (np.searchsorted(test_users, tu[rows]), ti[rows]))
    case = dict(name=name, n_users=n_users, n_items=n_items, rank=rank, epochs=epochs, neg_prop=neg_prop, seed=seed, triplets=(u, i, f),
                C=C, X=X, Y=Y, test_users=test_users, lists=lists, gaps=gaps)
    for a in (X, Y, lists, gaps):
        a.setflags(write=False)
    _cases[name] = case
    return case


def model_for(case, ops, cls=None, data=None, **kwargs):
    cls = lmf.ImplicitLMF if cls is None else cls
    u, i, f = case['triplets']
    m = cls(model_data(u, i, f, case['n_users'], case['n_items'], case['seed']) if data is None else data, seed=case['seed'], ops=ops,
            **kwargs)
    m.verbose = False
    m.rank, m.num_epochs, m.neg_prop, m.topk = case['rank'], case['epochs'], case['neg_prop'], TOPK
    return m


def warm_case(name='r14', n_new=25, seed=9):
    """New users for a warm start against the model of `model_case(name)`: 2 .. 10 known items each with feedback 1 .. 5 — the
    first one 1 (the default confidence log2(1) = 0: not folded in but still seen) — and one held-out item each."""
    case = model_case(name)
    rng = np.random.RandomState(seed)
    tu, ti, tf, hi = [], [], [], []
    for u in range(n_new):
        items = rng.permutation(case['n_items'])[:rng.randint(3, 12)]
        vals = rng.randint(1, 6, size=len(items) - 1).astype(np.float64)
        vals[0] = 1.0
        order = np.argsort(items[:-1])
        hi.append(items[-1])
        tu += [u] * len(order)
        ti += list(items[:-1][order])
        tf += list(vals[order])
    return dict(case=case, test=(np.array(tu, dtype=np.int64), np.array(ti, dtype=np.int64), np.array(tf)),
                holdout=(np.arange(n_new, dtype=np.int64), np.array(hi, dtype=np.int64), np.ones(n_new)), n_new=n_new)


def warm_data(w):
    from polara_amd.data import ArrayData
    case = w['case']
    base = model_data(*case['triplets'], case['n_users'], case['n_items'], case['seed'])
    return ArrayData(tuple(base.training), n_users=case['n_users'], n_items=case['n_items'], test=w['test'], holdout=w['holdout'],
                     warm_start=True, fields=('userid', 'itemid', 'rating'))
