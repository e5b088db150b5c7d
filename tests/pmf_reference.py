"""TEST-ONLY NumPy restatement of the blocked PMF sweep (plan, epoch, solver) with the DEVICE's summation orders, the CPU
double of the PMF operators, and the helpers that turn a tests/golden/pmf_*.npz fixture into inputs.  Never imported by the
package.

An epoch sweeps the strata one after the other; within a stratum the blocks are independent, so sample t of every block is
computed at once (element-wise NumPy: the same bits as one block after the other).  Per sample, in the order of
include/polara_hip.h: the products pm[c] qn[c] go into w = 16 / 32 / 64 slots (zeros beyond the rank) that are summed by a
halving tree; err, the two lambdas (as divisions), both gradients from the old rows, the adjustment of P then of Q, the
stores.  A block adds err^2 in sample order; the block sums of a stratum are added in block order, the stratum sums in
stratum order."""
import math

import numpy as np
import torch

from numpy_ops import NumpyOps
from polara_amd import pmf

MAX_RANK = 64
GAMMA, SMOOTHING = 0.9, 1e-6


def group_width(rank):
    return 16 if rank <= 16 else 32 if rank <= 32 else 64


def tree_dot(p, q, w):
    """rows of p * q summed by the halving tree over w slots"""
    d = np.zeros((p.shape[0], w))
    d[:, :p.shape[1]] = p * q
    h = w // 2
    while h >= 1:
        d = d[:, :h] + d[:, h:2 * h]
        h //= 2
    return d[:, 0]


def adjusted(kind, g, S, rows, gamma, smoothing):
    if kind is None:
        return g
    if kind == 'adagrad':
        u = S[rows] + g * g
    elif kind == 'rmsprop':
        u = gamma * S[rows] + (1 - gamma) * (g * g)
    else:
        raise ValueError(kind)
    S[rows] = u
    return g / np.sqrt(smoothing + u)


def make_plan(users, items, vals, n_users, n_items, blocks):
    """the plan dict of HipOps.pmf_plan as NumPy arrays, from canonical interactions"""
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    if (vals == 0).any():
        raise ValueError('PMF: an interaction with feedback 0 (after summing duplicates)')
    perm, block_ptr = pmf.block_schedule(users, items, n_users, n_items, blocks)
    return dict(blocks=int(blocks), nnz=len(users), shape=(int(n_users), int(n_items)), perm=perm, block_ptr=block_ptr,
                users=users[perm].astype(np.int32), items=items[perm].astype(np.int32), vals=vals[perm],
                row_nnz=np.bincount(users, minlength=n_users).astype(np.float64),
                col_nnz=np.bincount(items, minlength=n_items).astype(np.float64))


def epoch(plan, P, Q, eta, lambd, adjust=None, state=None, gamma=GAMMA, smoothing=SMOOTHING):
    """one sweep, P and Q (and the state) updated in place; returns the squared error"""
    B, bp = plan['blocks'], plan['block_ptr']
    users, items, vals, rnnz, cnnz = plan['users'], plan['items'], plan['vals'], plan['row_nnz'], plan['col_nnz']
    w = group_width(P.shape[1])
    SP, SQ = state if adjust else (None, None)
    block_sse = np.zeros((B, B))
    for s in range(B):
        starts = bp[s * B:(s + 1) * B]
        lens = bp[s * B + 1:(s + 1) * B + 1] - starts
        sse = np.zeros(B)
        for t in range(int(lens.max())):
            act = np.flatnonzero(t < lens)
            pos = starts[act] + t
            m, n, v = users[pos], items[pos], vals[pos]
            pm, qn = P[m], Q[n]
            err = v - tree_dot(pm, qn, w)
            row_lambda, col_lambda = lambd / rnnz[m], lambd / cnnz[n]
            gp = err[:, None] * qn - pm * row_lambda[:, None]
            gq = err[:, None] * pm - qn * col_lambda[:, None]
            P[m] = pm + eta * adjusted(adjust, gp, SP, m, gamma, smoothing)
            Q[n] = qn + eta * adjusted(adjust, gq, SQ, n, gamma, smoothing)
            sse[act] = sse[act] + err * err
        block_sse[s] = sse
    strata = np.add.accumulate(block_sse, axis=1)[:, -1]            # strictly left to right
    return float(np.add.accumulate(strata)[-1])


def solve(plan, P0, Q0, lrate, sigma, num_epochs, tol, adjust=None):
    """mf_sgd_boilerplate (optimize.py:158-220) on the restated epoch: (P, Q, RMSE history)"""
    P, Q = P0.copy(), Q0.copy()
    lambd = 0.5 * sigma ** 2
    last_err = np.finfo('f8').max
    history = []
    for _ in range(int(num_epochs)):
        state = (np.zeros_like(P), np.zeros_like(Q)) if adjust else None
        new_err = epoch(plan, P, Q, lrate, lambd, adjust, state)
        refined = abs(last_err - new_err) / last_err
        last_err = new_err
        history.append(math.sqrt(new_err / plan['nnz']))
        if refined < tol:
            break
    return P, Q, np.array(history)


def top_lists(scores, topk, seen=None):
    """rows of `scores` -> topk column ids by descending score, ties by ascending id; seen = (rows, cols) masked out"""
    s = scores.copy()
    if seen is not None:
        s[seen] = -np.inf
    return np.stack([np.lexsort((np.arange(s.shape[1]), -row))[:topk] for row in s]).astype(np.int64)


# ---- fixtures --------------------------------------------------------------------------------------------------------
def adjust_of(g):
    a = str(g['adjust'])
    return None if a == 'none' else a


def fixture_plan(g, blocks=None):
    idx, shp = g['train_idx'], tuple(int(x) for x in g['train_shape'])
    return make_plan(idx[:, 0], idx[:, 1], g['train_val'], shp[0], shp[1], int(g['blocks']) if blocks is None else blocks)


def solver_args(g):
    return dict(lrate=float(g['learn_rate']), sigma=float(g['sigma']), num_epochs=int(g['num_epochs']), tol=float(g['tolerance']),
                adjust=adjust_of(g))


def golden_data(g):
    from polara_amd.data import ArrayData
    idx, shp = g['train_idx'], tuple(int(x) for x in g['train_shape'])
    return ArrayData((idx[:, 0], idx[:, 1], g['train_val']), n_users=shp[0], n_items=shp[1],
                     holdout=(g['hold_user'], g['hold_item'], g['hold_fdbk']), fields=('userid', 'itemid', 'rating'))


def model_for(g, ops, data=None):
    m = pmf.ProbabilisticMF(golden_data(g) if data is None else data, seed=int(g['seed']), ops=ops)
    m.verbose = False
    m.rank, m.topk, m.blocks = int(g['rank']), int(g['topk']), int(g['blocks'])
    m.learn_rate, m.sigma, m.num_epochs, m.tolerance = float(g['learn_rate']), float(g['sigma']), int(g['num_epochs']), float(g['tolerance'])
    return m


# ---- the CPU double of the PMF operators --------------------------------------------------------------------------------
class PMFNumpyOps(NumpyOps):
    """NumpyOps plus what polara_amd/pmf.py asks of HipOps (same semantics on CPU tensors)."""

    def pmf_max_rank(self):
        return MAX_RANK

    def pmf_plan(self, A, blocks):
        m = A.m.tocsr()
        m.sort_indices()
        users = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(m.indptr))
        plan = make_plan(users, m.indices, m.data, A.shape[0], A.shape[1], blocks)
        return {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in plan.items()}

    def pmf_epoch(self, plan, P, Q, eta, lambd, adjust=None, state=None, gamma=GAMMA, smoothing=SMOOTHING):
        if int(P.shape[1]) > MAX_RANK:
            raise ValueError('PMF: rank %d outside 1..%d' % (P.shape[1], MAX_RANK))
        host = {k: v.numpy() if torch.is_tensor(v) else v for k, v in plan.items()}
        st = tuple(s.numpy() for s in state) if adjust else None
        return torch.tensor([epoch(host, P.numpy(), Q.numpy(), float(eta), float(lambd), adjust, st, gamma, smoothing)],
                            dtype=torch.float64)
