"""TEST-ONLY NumPy/SciPy restatement of Local Collective Embeddings, written from the update formulae in the TRANSPOSED
layout the device solver uses (W [n x k], HsT [v1 x k], HuT [v2 x k]), the CPU double of the LCE operators, and the
helpers that turn a tests/golden/lce_*.npz fixture into inputs.  Never imported by the package.

    HsT <- HsT o (a XsT W) / max(HsT (a WtW) + l HsT, 1e-10)            a = alpha
    HuT <- HuT o (g XuT W) / max(HuT (g WtW) + l HuT, 1e-10)            g = 1 - alpha
    W   <- W o (a Xs HsT + g Xu HuT + b A W) / max(W (a HsTt HsT + g HuTt HuT) + b d o W + l W, 1e-10)
    Obj = a (|Xs|^2 - 2 <HsT, XsT W> + <WtW, HsTt HsT>) + g (same with Xu, HuT) + b (<W, d o W> - <W, A W>)
          + l (tr WtW + |HsT|^2 + |HuT|^2)
"""
import numpy as np
import scipy.sparse as sps
import torch

from test_coldstart_host import ColdStartNumpyOps

FLOOR = 1e-10
FUSED_MAX_RANK = 128


def update(X, N, M, a, lamb, c=None):
    """X o (a N) / max(X M + (lamb + c_i) X, 1e-10)"""
    shift = lamb if c is None else (lamb + c)[:, None]
    return X * ((a * N) / np.maximum(X @ M + shift * X, FLOOR))


def solve(Xs, Xu, A, W0, Hs0, Hu0, alpha=0.1, beta=0.05, lamb=1., epsilon=1e-4, maxiter=15, user_perm=None):
    """Returns (W, HuT, HsT, objective history).  user_perm: run with the users in another order (a different summation
    order everywhere a sum runs over users); the rows of HuT come back in the original order."""
    Xs, Xu, A = (sps.csr_matrix(M, dtype=np.float64) for M in (Xs, Xu, A))
    W, HsT, HuT = W0.copy(), Hs0.T.copy(), Hu0.T.copy()
    if user_perm is not None:
        Xu, HuT = Xu[:, user_perm].tocsr(), HuT[user_perm]
    gamma = 1. - alpha
    d = np.asarray(A.sum(axis=0)).ravel()
    XsT, XuT = Xs.T.tocsr(), Xu.T.tocsr()
    const = alpha * Xs.multiply(Xs).sum() + gamma * Xu.multiply(Xu).sum()
    history = []
    it = 1
    G = W.T @ W
    Ns, Nu, AW = XsT @ W, XuT @ W, A @ W
    while True:
        HsT = update(HsT, Ns, alpha * G, alpha, lamb)
        HuT = update(HuT, Nu, gamma * G, gamma, lamb)
        Gs, Gu = HsT.T @ HsT, HuT.T @ HuT
        W = update(W, alpha * (Xs @ HsT) + gamma * (Xu @ HuT) + beta * AW, alpha * Gs + gamma * Gu, 1., lamb, beta * d)
        G = W.T @ W
        Ns, Nu, AW = XsT @ W, XuT @ W, A @ W
        obj = (const + alpha * (-2. * np.sum(HsT * Ns) + np.sum(G * Gs)) + gamma * (-2. * np.sum(HuT * Nu) + np.sum(G * Gu))
               + beta * (np.sum(W * (d[:, None] * W)) - np.sum(W * AW)) + lamb * (np.trace(G) + np.trace(Gs) + np.trace(Gu)))
        history.append(float(obj))
        if it > 1 and (it > maxiter or abs(history[-1] - history[-2]) < epsilon):
            break
        it += 1
    if user_perm is not None:
        back = np.empty_like(HuT)
        back[user_perm] = HuT
        HuT = back
    return W, HuT, HsT, history


def cold_scores(Fc, HsT, HuT):
    """max(F_cold HsT pinv(HsT^T HsT), 0) HuT^T: [n_cold x n_users]"""
    E = np.asarray(Fc @ HsT) @ np.linalg.pinv(HsT.T @ HsT)
    return np.maximum(E, 0.) @ HuT.T


def top_lists(scores, topk, seen=None):
    """rows of `scores` -> topk column ids by descending score, ties by ascending id; seen = (rows, cols) masked out"""
    s = scores.copy()
    if seen is not None:
        s[seen] = -np.inf
    return np.stack([np.lexsort((np.arange(s.shape[1]), -row))[:topk] for row in s]).astype(np.int64)


# ---- fixtures --------------------------------------------------------------------------------------------------------
def coo(g, key):
    shp = tuple(int(x) for x in g[key + '_shape'])
    val = g[key + '_val'] if key + '_val' in g else np.ones(len(g[key + '_row']))
    return sps.csr_matrix((val, (g[key + '_row'], g[key + '_col'])), shape=shp)


def inputs(g):
    """(Xs, Xu, A, (W0, Hs0, Hu0), solver keywords) of a fixture"""
    idx, shp = g['train_idx'], tuple(int(x) for x in g['train_shape'])
    train = sps.csr_matrix((g['train_val'], (idx[:, 0], idx[:, 1])), shape=shp)
    kw = dict(alpha=float(g['alpha']), beta=float(g['beta']), lamb=float(g['regularization']), epsilon=float(g['tolerance']),
              maxiter=int(g['max_iterations']))
    return coo(g, 'ft'), train.T.tocsr(), coo(g, 'graph'), (g['W0'], g['Hs0'], g['Hu0']), kw


def golden_data(g):
    """the data object of a fixture: item cold start (the item column is called `item`, as in the fixtures) or standard"""
    from polara_amd.data import ArrayData, ItemColdStartArrayData
    idx, shp = g['train_idx'], tuple(int(x) for x in g['train_shape'])
    train = (idx[:, 0], idx[:, 1], g['train_val'])
    fields = ('userid', 'item', 'rating')
    if bool(g['cold_start']):
        return ItemColdStartArrayData(train, (g['hold_user'], g['hold_cold'], g['hold_fdbk']), coo(g, 'ft'), coo(g, 'fc'),
                                      n_users=shp[0], n_items=shp[1], fields=fields,
                                      representative_users=g['repr_users'] if 'repr_users' in g else None)
    return ArrayData(train, n_users=shp[0], n_items=shp[1], holdout=(g['hold_user'], g['hold_item'], g['hold_fdbk']),
                     fields=fields)


def model_for(g, ops, data=None):
    from polara_amd import lce
    data = golden_data(g) if data is None else data
    cold = bool(g['cold_start'])
    m = (lce.LCEModelItemColdStart if cold else lce.LCEModel)(data, ops=ops, **({} if cold else {'item_features': coo(g, 'ft')}))
    m.verbose = False
    m.rank, m.topk, m.seed = int(g['rank']), int(g['topk']), int(g['seed'])
    m.alpha, m.beta, m.regularization = float(g['alpha']), float(g['beta']), float(g['regularization'])
    m.tolerance, m.max_iterations = float(g['tolerance']), int(g['max_iterations'])
    m.binary_features = bool(g['binary_features'])
    m.item_graph = coo(g, 'graph')          # kNN over binary features is full of exact distance ties: the reference's own graph
    return m


# ---- the CPU double of the LCE operators --------------------------------------------------------------------------------
class LCENumpyOps(ColdStartNumpyOps):
    """ColdStartNumpyOps plus what polara_amd/lce.py asks of HipOps (same semantics on CPU tensors); the composed and the
    fused update are one formula here."""

    def lce_fused_max_rank(self):
        return FUSED_MAX_RANK

    def csr_scaled(self, A, s):
        return self.csr(A.m.indptr, A.m.indices, A.m.data * float(s), A.shape)

    def csr_values(self, A):
        return torch.from_numpy(np.asarray(A.m.data, dtype=np.float64))

    def spmm_acc(self, A, X, out):
        out += torch.from_numpy(np.ascontiguousarray(A.m @ X.numpy()))
        return out

    def lce_update(self, X, N, M1, ma=1.0, M2=None, mb=0.0, a=1.0, lamb=0.0, c=None, fused=None):
        M = ma * M1.numpy() + (mb * M2.numpy() if M2 is not None else 0.)
        X.copy_(torch.from_numpy(update(X.numpy(), N.numpy(), M, a, lamb, None if c is None else c.numpy())))
        return X

    def lce_dots(self, pairs, bias=0.0):
        out = torch.zeros(1 + len(pairs), dtype=torch.float64)
        for p, (coef, P, Q, w) in enumerate(pairs):
            v = P if Q is None else P * Q
            if w is not None:
                v = v * w[:, None]
            out[1 + p] = v.sum()
        out[0] = bias + sum(float(pairs[p][0]) * float(out[1 + p]) for p in range(len(pairs)))
        return out

    def clamp_min(self, E, lo=0.0):
        return E.clamp_(min=lo)
