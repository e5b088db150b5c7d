"""TEST-ONLY NumPy restatement of the kernelized PMF sweep (plan, epoch, solver) with the DEVICE's arithmetic
(include/polara_hip.h), the CPU double of the KPMF operators, and the helpers that turn a tests/golden/kpmf_*.npz fixture into
inputs.  Never imported by the package.

Everything is pmf_reference.py except the two gradients: per sample the neighbour sum of the user's row of Ku and of the item's
row of Ki — over the stored off-diagonal entries in storage order, every product and every sum rounded on its own, starting
from +0.0 — whose rows are read live when they lie in the block's own part and from the stratum's snapshot otherwise; the
diagonal term du[m] * (pm + pm) is added last.  Within a stratum the blocks are independent GIVEN the snapshot (a block reads
live only what it alone writes), so sample t of every block is computed at once as in pmf_reference.py."""
import math

import numpy as np
import scipy.sparse as sps
import torch

import pmf_reference as base
from pmf_reference import GAMMA, MAX_RANK, SMOOTHING, adjust_of, adjusted, group_width, solver_args, top_lists, tree_dot
from polara_amd import kpmf, pmf


def make_plan(users, items, vals, n_users, n_items, blocks, Ku, Ki):
    """the plan dict of HipOps.kpmf_plan as NumPy arrays, from canonical interactions and the two kernel matrices"""
    plan = base.make_plan(users, items, vals, n_users, n_items, blocks)
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    nnz = len(users)
    plan['user_part'] = pmf._parts(np.bincount(users, minlength=n_users), blocks, nnz).astype(np.int32)
    plan['item_part'] = pmf._parts(np.bincount(items, minlength=n_items), blocks, nnz).astype(np.int32)
    for side, K, n in (('ku', Ku, n_users), ('ki', Ki, n_items)):
        plan[side + '_ptr'], plan[side + '_idx'], plan[side + '_val'], plan[side + '_diag'] = kpmf.split_kernel(K, n)
    return plan


def neighbour_sum(ptr, idx, val, part, my_part, X, S, r, live=True):
    """(+0.0 + K[e1] X(j1)) + K[e2] X(j2) + ... over row r's off-diagonal entries, strictly left to right; X(j) is row j of X
    when `live` and j lies in my_part, row j of the snapshot S otherwise"""
    lo, hi = ptr[r], ptr[r + 1]
    j = idx[lo:hi]
    rows = np.where((part[j] == my_part)[:, None], X[j], S[j]) if live else S[j]
    terms = np.zeros((hi - lo + 1, X.shape[1]))
    terms[1:] = val[lo:hi, None] * rows
    return np.add.accumulate(terms, axis=0)[-1]


def epoch(plan, P, Q, eta, lambd, adjust=None, state=None, gamma=GAMMA, smoothing=SMOOTHING, live=True, cache=True, snapshots=None):
    """one sweep, P and Q (and the state) updated in place; returns the squared error.  live=False reads every neighbour row
    from the snapshot (NOT the device's semantics: what the fixtures must be able to tell apart).  cache=False computes the
    user's neighbour sum for every sample instead of once per run of a user.  snapshots: a list that receives (P_snap,
    Q_snap) as the device leaves them."""
    B, bp = plan['blocks'], plan['block_ptr']
    users, items, vals, rnnz, cnnz = plan['users'], plan['items'], plan['vals'], plan['row_nnz'], plan['col_nnz']
    upart, ipart = plan['user_part'], plan['item_part']
    ku = (plan['ku_ptr'], plan['ku_idx'], plan['ku_val'])
    ki = (plan['ki_ptr'], plan['ki_idx'], plan['ki_val'])
    du, di = plan['ku_diag'], plan['ki_diag']
    k = P.shape[1]
    w = group_width(k)
    SP, SQ = state if adjust else (None, None)
    block_sse = np.zeros((B, B))
    for s in range(B):
        PS, QS = P.copy(), Q.copy()                                    # the snapshot: P and Q as the stratum finds them
        starts = bp[s * B:(s + 1) * B]
        lens = bp[s * B + 1:(s + 1) * B + 1] - starts
        sse = np.zeros(B)
        last_user = np.full(B, -1)
        cached = np.zeros((B, k))
        for t in range(int(lens.max())):
            act = np.flatnonzero(t < lens)
            pos = starts[act] + t
            m, n, v = users[pos], items[pos], vals[pos]
            off_p, off_q = np.empty((len(act), k)), np.empty((len(act), k))
            for x, b in enumerate(act):
                if not cache or last_user[b] != m[x]:
                    cached[b] = neighbour_sum(*ku, upart, b, P, PS, m[x], live)
                    last_user[b] = m[x]
                off_p[x] = cached[b]
                off_q[x] = neighbour_sum(*ki, ipart, (b + s) % B, Q, QS, n[x], live)
            pm, qn = P[m], Q[n]
            err = v - tree_dot(pm, qn, w)
            row_lambda, col_lambda = lambd / rnnz[m], lambd / cnnz[n]
            kp = off_p + du[m][:, None] * (pm + pm)
            kq = off_q + di[n][:, None] * (qn + qn)
            gp = err[:, None] * qn - kp * row_lambda[:, None]
            gq = err[:, None] * pm - kq * col_lambda[:, None]
            P[m] = pm + eta * adjusted(adjust, gp, SP, m, gamma, smoothing)
            Q[n] = qn + eta * adjusted(adjust, gq, SQ, n, gamma, smoothing)
            sse[act] = sse[act] + err * err
        block_sse[s] = sse
    if snapshots is not None:
        snapshots[:] = [P.copy(), Q.copy()]
    strata = np.add.accumulate(block_sse, axis=1)[:, -1]            # strictly left to right
    return float(np.add.accumulate(strata)[-1])


def solve(plan, P0, Q0, lrate, sigma, num_epochs, tol, adjust=None, live=True):
    """mf_sgd_boilerplate (optimize.py:158-220) on the restated epoch: (P, Q, RMSE history)"""
    P, Q = P0.copy(), Q0.copy()
    lambd = 0.5 * sigma ** 2
    last_err = np.finfo('f8').max
    history = []
    for _ in range(int(num_epochs)):
        state = (np.zeros_like(P), np.zeros_like(Q)) if adjust else None
        new_err = epoch(plan, P, Q, lrate, lambd, adjust, state, live=live)
        refined = abs(last_err - new_err) / last_err
        last_err = new_err
        history.append(math.sqrt(new_err / plan['nnz']))
        if refined < tol:
            break
    return P, Q, np.array(history)


# ---- fixtures --------------------------------------------------------------------------------------------------------
def triplets_matrix(g, key, n):
    """a SciPy CSR from the fixture's `<key>_row / _col / _val` in their stored order, or None when the fixture has none"""
    if key + '_val' not in g:
        return None
    return sps.csr_matrix((g[key + '_val'], (g[key + '_row'], g[key + '_col'])), shape=(n, n))


def fixture_kernels(g):
    """(Ku, Ki) as the reference's optimizer received them"""
    n_users, n_items = (int(x) for x in g['train_shape'])
    return triplets_matrix(g, 'ku', n_users), triplets_matrix(g, 'ki', n_items)


def fixture_plan(g, blocks=None):
    idx, shp = g['train_idx'], tuple(int(x) for x in g['train_shape'])
    return make_plan(idx[:, 0], idx[:, 1], g['train_val'], shp[0], shp[1], int(g['blocks']) if blocks is None else blocks,
                     *fixture_kernels(g))


def golden_data(g):
    """SimilarityArrayData with the fixture's relations in the model's own id order"""
    from polara_amd.data import SimilarityArrayData
    idx, shp = g['train_idx'], tuple(int(x) for x in g['train_shape'])
    rel = {'userid': triplets_matrix(g, 'rel_u', shp[0]), 'itemid': triplets_matrix(g, 'rel_i', shp[1])}
    return SimilarityArrayData((idx[:, 0], idx[:, 1], g['train_val']), n_users=shp[0], n_items=shp[1],
                               holdout=(g['hold_user'], g['hold_item'], g['hold_fdbk']), fields=('userid', 'itemid', 'rating'),
                               relations_matrices=rel, relations_indices={'userid': None, 'itemid': None})


def model_for(g, ops, data=None):
    m = kpmf.KernelizedPMF(golden_data(g) if data is None else data, seed=int(g['seed']), ops=ops)
    m.verbose = False
    m.rank, m.topk, m.blocks = int(g['rank']), int(g['topk']), int(g['blocks'])
    m.learn_rate, m.sigma, m.num_epochs, m.tolerance = float(g['learn_rate']), float(g['sigma']), int(g['num_epochs']), float(g['tolerance'])
    m.gamma = float(g['gamma'])
    m.factor_sigma = {'userid': float(g['factor_sigma_user']), 'itemid': float(g['factor_sigma_item'])}
    return m


# ---- the CPU double of the KPMF operators -------------------------------------------------------------------------------
class KPMFNumpyOps(base.PMFNumpyOps):
    """PMFNumpyOps plus what polara_amd/kpmf.py asks of HipOps (same semantics on CPU tensors)."""

    def kpmf_plan(self, A, blocks, Ku, Ki):
        m = A.m.tocsr()
        m.sort_indices()
        users = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(m.indptr))
        plan = make_plan(users, m.indices, m.data, A.shape[0], A.shape[1], blocks, Ku, Ki)
        return {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in plan.items()}

    def kpmf_epoch(self, plan, P, Q, eta, lambd, adjust=None, state=None, gamma=GAMMA, smoothing=SMOOTHING, snapshots=None):
        if int(P.shape[1]) > MAX_RANK:
            raise ValueError('KPMF: rank %d outside 1..%d' % (P.shape[1], MAX_RANK))
        host = {k: v.numpy() if torch.is_tensor(v) else v for k, v in plan.items()}
        st = tuple(s.numpy() for s in state) if adjust else None
        snaps = []
        sse = epoch(host, P.numpy(), Q.numpy(), float(eta), float(lambd), adjust, st, gamma, smoothing, snapshots=snaps)
        if snapshots is not None:
            for dst, src in zip(snapshots, snaps):
                dst.copy_(torch.from_numpy(src))
        return torch.tensor([sse], dtype=torch.float64)
