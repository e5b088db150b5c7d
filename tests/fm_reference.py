"""TEST-ONLY NumPy restatement of the factorisation model with side features (polara_amd/fm.py, csrc/fm.hip; the specification
is the comment in include/polara_hip.h): features, plan, the label image, the sample, the label step, the epoch and the fit, in
schedule order — a blocked stratum IS the serial sweep over its positions, because its blocks share no row they write and the
label rows are read-only while it runs.  It borrows PMF's plan (pmf_reference.make_plan) and the halving tree of
bpr_reference.  Never imported by the package.

No equality with any build of turicreate is claimed; interactions inside one side are not modelled (see polara_amd/fm.py)."""
import math

import numpy as np

import pmf_reference as pref
from bpr_reference import group_width, top_lists, tree_sum  # noqa: F401

MAX_RANK = 62
SMOOTHING = 1e-6
FEATURE_KEYS = ('a', 'row_ptr', 'row_idx', 'row_val', 'col_ptr', 'col_idx', 'col_val')


# ---- features, plan, initial parameters ----------------------------------------------------------------------------------------
def make_features(one_hot, normalize=False):
    """dense 0/1 [n_rows x n_labels] -> a [n_rows] (1, or 1 / (1 + labels of the row)) and F = diag(a) one_hot as CSR (row_*)
    and CSC (col_*), indices ascending"""
    one_hot = (np.asarray(one_hot) != 0)
    n_rows, n_labels = one_hot.shape
    a = 1.0 / (1.0 + one_hot.sum(1).astype(np.float64)) if normalize else np.ones(n_rows)
    rows, cols = np.nonzero(one_hot)
    by_col = np.lexsort((rows, cols))
    ptr = lambda idx, n: np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n))]).astype(np.int64)
    return dict(n_labels=n_labels, a=a, row_ptr=ptr(rows, n_rows), row_idx=cols.astype(np.int32), row_val=a[rows],
                col_ptr=ptr(cols, n_labels), col_idx=rows[by_col].astype(np.int32), col_val=a[rows[by_col]])


def make_plan(ratings, blocks, hot_users=None, hot_items=None, normalize=False):
    """the plan dict of HipOps.fm_plan as NumPy arrays from a dense rating matrix (0: no rating) and dense one-hot matrices"""
    users, items = np.nonzero(ratings)
    plan = pref.make_plan(users, items, ratings[users, items], ratings.shape[0], ratings.shape[1], blocks)
    plan['features'] = dict(user=None if hot_users is None else make_features(hot_users, normalize),
                            item=None if hot_items is None else make_features(hot_items, normalize))
    return plan


def initial_parameters(n_users, n_items, n_ulabels, n_ilabels, rank, seed):
    rnds = np.random.RandomState(seed)
    out = []
    for n in (n_users, n_items, n_ulabels, n_ilabels):
        X = np.zeros((n, rank + 2))
        X[:, :rank] = rnds.normal(scale=0.1, size=(n, rank))
        out.append(X)
    out[0][:, rank + 1] = 1.0
    out[1][:, rank] = 1.0
    return tuple(out)


# ---- the pieces ---------------------------------------------------------------------------------------------------------------
def label_image(feat, L):
    """S = F L: per row (+0.0 + v1 * L[l1]) + v2 * L[l2] + ... in storage order"""
    n_rows = len(feat['a'])
    S = np.zeros((n_rows, L.shape[1]))
    for r in range(n_rows):
        for e in range(feat['row_ptr'][r], feat['row_ptr'][r + 1]):
            S[r] = S[r] + feat['row_val'][e] * L[feat['row_idx'][e]]
    return S


def adjusted(kind, g, s, gamma, smoothing):
    """(adj(g), the new state) elementwise: PMF's adjusters"""
    if kind is None:
        return g, s
    if kind == 'adagrad':
        u = s + g * g
    elif kind == 'rmsprop':
        u = gamma * s + (1.0 - gamma) * (g * g)
    else:
        raise ValueError(kind)
    return g / np.sqrt(smoothing + u), u


def take_step(X, S, r, cols, g, step, adjust, gamma, smoothing):
    """the step rule on the columns `cols` (a boolean mask) of row r of X with the gradient g, state S (None without adjuster)"""
    adj, u = adjusted(adjust, g, S[r] if adjust else None, gamma, smoothing)
    X[r, cols] = (X[r] - step * adj)[cols]
    if adjust:
        S[r, cols] = u[cols]


def lambdas(k, reg, lin_reg):
    lam = np.full(k + 2, float(lin_reg))
    lam[:k] = float(reg)
    return lam


def stepped_columns(k, item_side, labels=False, label_factors=True):
    """the columns of a row that are ever stepped: the factors (not those of label rows when the side data is not factorised)
    and the side's own bias column — k for the user side, k + 1 for the item side"""
    c = np.arange(k + 2)
    factors = (c < k) & (label_factors or not labels)
    return factors | (c == (k + 1 if item_side else k))


def representations(plan, P, E, LU, LI):
    fu, fi = plan['features']['user'], plan['features']['item']
    Pt = P.copy() if fu is None else fu['a'][:, None] * P + label_image(fu, LU)
    Qt = E.copy() if fi is None else fi['a'][:, None] * E + label_image(fi, LI)
    return Pt, Qt


def sample(pu, ei, r, mean, w, lam, au=None, su=None, ai=None, si=None):
    """(err, eq, ep, gp, gq) of one sample from the two identity rows before the update; au / su (ai / si): the weight and the
    image row of the user (item) with features on that side, None without"""
    pt = pu if au is None else au * pu + su
    qt = ei if ai is None else ai * ei + si
    err = (mean + tree_sum(pt * qt, w)) - r
    eq, ep = err * qt, err * pt
    gp = (eq if au is None else au * eq) + lam * pu
    gq = (ep if ai is None else ai * ep) + lam * ei
    return err, eq, ep, gp, gq


def label_gradient(feat, G, L, l, lam):
    """(g_l + (lambda * N_l) * L[l] over all C columns, N_l) of label l from the rows of G [n_rows x (C + 1)]"""
    C = L.shape[1]
    g, N = np.zeros(C), 0.0
    for e in range(feat['col_ptr'][l], feat['col_ptr'][l + 1]):
        row = G[feat['col_idx'][e]]
        g = g + feat['col_val'][e] * row[:C]
        N = N + row[C]
    return g + (lam * N) * L[l], N


def label_step(feat, G, L, SL, item_side, step, reg, lin_reg, adjust=None, gamma=0.9, label_factors=True, smoothing=SMOOTHING,
               clear=True):
    """g_l = (+0.0 + v1 * G[r1]) + v2 * G[r2] + ... and N_l the summed counts (column C of G) over the label's rows ascending;
    a label with N_l = 0 is left alone; g_l + (lambda * N_l) * L[l], one step on the stepped columns; G is zeroed"""
    k = L.shape[1] - 2
    lam, cols = lambdas(k, reg, lin_reg), stepped_columns(k, item_side, True, label_factors)
    for l in range(feat['n_labels']):
        g, N = label_gradient(feat, G, L, l, lam)
        if N == 0.0:
            continue
        take_step(L, SL, l, cols, g, step, adjust, gamma, smoothing)
    if clear:
        G[...] = 0.0


# ---- the epoch ----------------------------------------------------------------------------------------------------------------
def epoch(plan, mean, P, E, LU, LI, state, step, reg, lin_reg, adjust=None, gamma=0.9, label_factors=True, smoothing=SMOOTHING):
    """one sweep in schedule order, everything updated in place; returns the squared error (block sums in sample order, added
    per stratum in block order and then in stratum order)"""
    k = P.shape[1] - 2
    C = k + 2
    w = group_width(C)
    B, bp = plan['blocks'], plan['block_ptr']
    users, items, vals = plan['users'], plan['items'], plan['vals']
    fu, fi = plan['features']['user'], plan['features']['item']
    lam = lambdas(k, reg, lin_reg)
    up, uq = stepped_columns(k, False), stepped_columns(k, True)
    SP, SE, SLU, SLI = state if adjust else (None,) * 4
    GU = None if fu is None else np.zeros((P.shape[0], C + 1))
    GI = None if fi is None else np.zeros((E.shape[0], C + 1))
    block_sse = np.zeros((B, B))
    for s in range(B):
        SU = None if fu is None else label_image(fu, LU)
        SI = None if fi is None else label_image(fi, LI)
        for b in range(B):
            sse = 0.0
            for p in range(bp[s * B + b], bp[s * B + b + 1]):
                u, i, r = users[p], items[p], vals[p]
                pu, ei = P[u].copy(), E[i].copy()
                err, eq, ep, gp, gq = sample(pu, ei, r, mean, w, lam, *((None, None) if fu is None else (fu['a'][u], SU[u])),
                                             *((None, None) if fi is None else (fi['a'][i], SI[i])))
                take_step(P, SP, u, up, gp, step, adjust, gamma, smoothing)
                take_step(E, SE, i, uq, gq, step, adjust, gamma, smoothing)
                if fu is not None:
                    GU[u, :C] = GU[u, :C] + eq
                    GU[u, C] = GU[u, C] + 1.0
                if fi is not None:
                    GI[i, :C] = GI[i, :C] + ep
                    GI[i, C] = GI[i, C] + 1.0
                sse = sse + err * err
            block_sse[s, b] = sse
        if fu is not None:
            label_step(fu, GU, LU, SLU, False, step, reg, lin_reg, adjust, gamma, label_factors, smoothing)
        if fi is not None:
            label_step(fi, GI, LI, SLI, True, step, reg, lin_reg, adjust, gamma, label_factors, smoothing)
    strata = np.add.accumulate(block_sse, axis=1)[:, -1]            # strictly left to right
    return float(np.add.accumulate(strata)[-1])


def step_rule(solver='auto', adagrad_momentum_weighting=0.9, sgd_step_size=0):
    adjust, gamma = None, 0.9
    if solver != 'sgd':
        adjust = 'adagrad' if adagrad_momentum_weighting is None else 'rmsprop'
        gamma = 0.9 if adagrad_momentum_weighting is None else float(adagrad_momentum_weighting)
    step = float(sgd_step_size) if sgd_step_size else (0.05 if adjust else 0.005)
    return adjust, gamma, step


def fit(ratings, rank, num_epochs, seed, blocks, hot_users=None, hot_items=None, normalize=False, regularization=1e-10,
        linear_regularization=1e-10, solver='auto', adagrad_momentum_weighting=0.9, sgd_step_size=0, label_factors=True, init=None,
        mean=None):
    """fm.fm_fit restated: dict of the four blocks (LU / LI None without features), the representations, the states, the RMSE
    history and the mean"""
    n_users, n_items = ratings.shape
    plan = make_plan(ratings, blocks, hot_users, hot_items, normalize)
    mean = float(np.mean(ratings[np.nonzero(ratings)])) if mean is None else float(mean)
    adjust, gamma, step = step_rule(solver, adagrad_momentum_weighting, sgd_step_size)
    n_ul, n_il = (0 if h is None else np.asarray(h).shape[1] for h in (hot_users, hot_items))
    P, E, LU, LI = (x.copy() for x in (initial_parameters(n_users, n_items, n_ul, n_il, rank, seed) if init is None else init))
    if not label_factors:                                             # the label factor columns stay 0
        LU[:, :rank] = 0.0
        LI[:, :rank] = 0.0
    state = tuple(np.zeros_like(x) for x in (P, E, LU, LI)) if adjust else None
    history = []
    for _ in range(num_epochs):
        sse = epoch(plan, mean, P, E, LU if hot_users is not None else None, LI if hot_items is not None else None, state, step,
                    regularization, linear_regularization, adjust, gamma, label_factors)
        history.append(math.sqrt(sse / plan['nnz']))
    Pt, Qt = representations(plan, P, E, LU, LI)
    return dict(P=P, E=E, LU=LU if hot_users is not None else None, LI=LI if hot_items is not None else None, Pt=Pt, Qt=Qt,
                state=state, history=history, mean=mean, plan=plan)


def cold_queries(cold_one_hot, LI, normalize=False):
    """w (e_k + sum of the label rows of a cold item's known labels), storage order; w = 1, or 1 / (1 + m) when normalised"""
    cold_one_hot = np.asarray(cold_one_hot) != 0
    k = LI.shape[1] - 2
    out = np.zeros((cold_one_hot.shape[0], LI.shape[1]))
    for i, row in enumerate(cold_one_hot):
        labels = np.flatnonzero(row)
        w = 1.0 / (1.0 + len(labels)) if normalize else 1.0
        for l in labels:
            out[i] = out[i] + w * LI[l]
        out[i, k] = w
    return out


# ---- the CPU double of the operators --------------------------------------------------------------------------------------------
def numpy_ops():
    """NumpyOps plus what polara_amd/fm.py asks of HipOps (same semantics on CPU tensors)"""
    import torch
    from numpy_ops import NumpyOps

    def host(x):
        return None if x is None else x.numpy()

    def tensors(d):
        return {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else tensors(v) if isinstance(v, dict) else v for k, v in d.items()}

    def arrays(d):
        return {k: v.numpy() if torch.is_tensor(v) else arrays(v) if isinstance(v, dict) else v for k, v in d.items()}

    class FMNumpyOps(NumpyOps):
        def fm_max_rank(self):
            return MAX_RANK

        def csr_values_host(self, A):
            m = A.m.tocsr()
            m.sort_indices()
            return np.asarray(m.data, dtype=np.float64)

        def fm_plan(self, A, blocks, user_features=None, item_features=None, normalize=False):
            dense = np.asarray(A.m.toarray(), dtype=np.float64)
            return tensors(make_plan(dense, blocks, None if user_features is None else user_features.toarray(),
                                     None if item_features is None else item_features.toarray(), normalize))

        def fm_label_image(self, plan, side, L):
            return torch.from_numpy(label_image(arrays(plan['features'][side]), L.numpy()))

        def fm_representation(self, plan, side, X, L=None):
            f = plan['features'][side]
            if f is None:
                return X.clone()
            f = arrays(f)
            return torch.from_numpy(f['a'][:, None] * X.numpy() + label_image(f, L.numpy()))

        def fm_label_step(self, plan, side, G, L, SL, step, reg, lin_reg, adjust=None, gamma=0.9, label_factors=True,
                          smoothing=SMOOTHING):
            label_step(arrays(plan['features'][side]), G.numpy(), L.numpy(), host(SL), side == 'item', float(step), reg, lin_reg,
                       adjust, gamma, label_factors, smoothing)

        def fm_epoch(self, plan, mean, P, E, LU, LI, state, step, reg, lin_reg, adjust=None, gamma=0.9, work=None,
                     label_factors=True, smoothing=SMOOTHING):
            if int(P.shape[1]) - 2 > MAX_RANK:
                raise ValueError('TCF: rank %d outside 1..%d' % (P.shape[1] - 2, MAX_RANK))
            st = tuple(host(s) for s in state) if adjust else None
            return torch.tensor([epoch(arrays(plan), float(mean), P.numpy(), E.numpy(), host(LU), host(LI), st, float(step), reg,
                                       lin_reg, adjust, gamma, label_factors, smoothing)], dtype=torch.float64)

    return FMNumpyOps()


# ---- test matrices --------------------------------------------------------------------------------------------------------------
def random_ratings(n_users=37, n_items=23, density=0.3, seed=0):
    """dense ratings 1..5 (0: none), about 30 % of the cells"""
    rng = np.random.RandomState(seed)
    return (rng.rand(n_users, n_items) < density) * rng.randint(1, 6, size=(n_users, n_items)).astype(np.float64)


def random_hot(n_rows, n_labels, seed):
    """0/1 [n_rows x n_labels]: about two labels per row, row 0 with none, label 0 on every other row, the last label on no row"""
    hot = (np.random.RandomState(seed).rand(n_rows, n_labels) < 0.3).astype(np.int8)
    hot[:, 0] = 1
    hot[0] = 0
    hot[:, n_labels - 1] = 0
    return hot


def planted_ratings(seed=2, n_users=60, n_items=40, n_cold=8, rank=2, n_ulabels=4, n_ilabels=5, density=0.25, noise=0.1):
    """A planted rating model: mu + user bias + item bias + a label effect per side + <p_u, q_i> with p, q sums of an identity
    part and label parts, plus noise.  Returns a dict: train (dense, 0: none), holdout triplets (one rating per user taken out
    of the training matrix), the one-hot matrices of users and warm items, and for `n_cold` further items their one-hot
    rows and their (user, cold item, rating) triplets."""
    rng = np.random.RandomState(seed)
    n_all = n_items + n_cold
    hot_u = np.zeros((n_users, n_ulabels), dtype=np.int8)
    hot_u[np.arange(n_users), rng.randint(n_ulabels, size=n_users)] = 1
    hot_i = np.zeros((n_all, n_ilabels), dtype=np.int8)
    hot_i[np.arange(n_all), rng.randint(n_ilabels, size=n_all)] = 1
    hot_i[np.arange(n_all), rng.randint(n_ilabels, size=n_all)] = 1
    bu, bi = rng.normal(scale=0.3, size=n_users), rng.normal(scale=0.2, size=n_all)
    wu, wi = rng.normal(scale=0.3, size=n_ulabels), rng.normal(scale=0.7, size=n_ilabels)
    p = rng.normal(scale=0.3, size=(n_users, rank)) + hot_u @ rng.normal(scale=0.6, size=(n_ulabels, rank))
    q = rng.normal(scale=0.3, size=(n_all, rank)) + hot_i @ rng.normal(scale=0.6, size=(n_ilabels, rank))
    full = 3.5 + bu[:, None] + bi[None, :] + (hot_u @ wu)[:, None] + (hot_i @ wi)[None, :] + p @ q.T
    full = full + rng.normal(scale=noise, size=full.shape)
    seen = rng.rand(n_users, n_all) < density
    seen[np.arange(n_users), rng.randint(n_items, size=n_users)] = True           # every user rates a warm item ...
    seen[np.arange(n_users), rng.randint(n_items, size=n_users)] = True           # ... or two
    train = np.where(seen[:, :n_items], full[:, :n_items], 0.0)
    hold_items = np.empty(n_users, dtype=np.int64)
    for u in range(n_users):
        rated = np.flatnonzero(train[u])
        hold_items[u] = rated[rng.randint(len(rated))] if len(rated) > 1 else -1
    users = np.flatnonzero(hold_items >= 0)
    holdout = (users, hold_items[users], train[users, hold_items[users]].copy())
    train[users, hold_items[users]] = 0.0
    fans, cold_items = np.nonzero(seen[:, n_items:])
    return dict(train=train, holdout=holdout, hot_users=hot_u, hot_items=hot_i[:n_items], cold_hot=hot_i[n_items:],
                cold=(fans, cold_items, full[fans, n_items + cold_items]), full=full)
