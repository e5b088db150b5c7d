"""TEST-ONLY NumPy restatement of the WARP model (polara_amd/warp.py, csrc/warp.hip; the specification is the comment in
include/polara_hip.h): features, loss table, candidates, the label image, the sample, the label step, the epoch and the fit, in
schedule order — a blocked stratum IS the serial sweep over its positions, because its blocks share no row they write and the
label embeddings are read-only while it runs.  It plays the role bpr_reference.py plays for BPR and borrows its schedule, item
order, splitmix64 stream and halving tree.  Never imported by the package.

No equality with any build of the `lightfm` package is claimed.  Against it: fp64, not float32; every stored positive is visited
once per epoch in schedule order (LightFM shuffles them); candidates are uniform inside the epoch's item part, not the whole
catalogue; the draws are a predrawn counter stream, not a generator advanced in the loop; the rank estimate
floor((n_items - 1) / draws) uses n_items - 1 although the draws come from a part; the label embeddings step once per stratum
on the stratum's summed gradient instead of once per sample; there is no regularisation (item_alpha = user_alpha = 0); WARP
and adagrad only.

Below the restatement, `naive_epoch`: a second, deliberately naive loop over blocks and CSR rows with Python floats and dense
feature loops.  It shares nothing with the restatement but `mix64` / `stream_key`."""
import math

import numpy as np

from bpr_reference import (MASK, group_width, holdout_auc, item_order, make_plan, mix64, random_matrix, stream_key,  # noqa: F401
                           top_lists, tree_sum)

MAX_RANK = 63
MAX_SAMPLED = 64


# ---- features, loss table, initial embeddings ---------------------------------------------------------------------------------
def make_features(one_hot):
    """dense 0/1 [n_items x n_labels] -> a [n_items] = 1 / (1 + labels of the item) and F_lab = diag(a) one_hot as CSR (row_*)
    and CSC (col_*), indices ascending"""
    one_hot = (np.asarray(one_hot) != 0)
    n_items, n_labels = one_hot.shape
    a = 1.0 / (1.0 + one_hot.sum(1).astype(np.float64))
    rows, cols = np.nonzero(one_hot)
    by_col = np.lexsort((rows, cols))
    ptr = lambda idx, n: np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n))]).astype(np.int64)
    return dict(n_labels=n_labels, a=a, row_ptr=ptr(rows, n_items), row_idx=cols.astype(np.int32), row_val=a[rows],
                col_ptr=ptr(cols, n_labels), col_idx=rows[by_col].astype(np.int32), col_val=a[rows[by_col]])


def loss_table(n_items, max_sampled):
    t = np.arange(int(max_sampled), dtype=np.float64)
    return np.minimum(10.0, np.log(np.maximum(1.0, np.floor((int(n_items) - 1) / (t + 1)))))


def initial_embeddings(n_users, n_items, n_labels, rank, seed):
    rnds = np.random.RandomState(seed)
    P, E, L = np.ones((n_users, rank + 1)), np.zeros((n_items, rank + 1)), np.zeros((n_labels, rank + 1))
    P[:, :rank] = (rnds.rand(n_users, rank) - 0.5) / rank
    E[:, :rank] = (rnds.rand(n_items, rank) - 0.5) / rank
    L[:, :rank] = (rnds.rand(n_labels, rank) - 0.5) / rank
    return P, E, L


# ---- candidates ---------------------------------------------------------------------------------------------------------------
def draw_candidates(plan, seed, epoch, max_sampled):
    """int32 [nnz x D]: the D candidates of every position of the schedule; one that lies in the user's row is -1"""
    D = int(max_sampled)
    h = stream_key(seed, epoch)
    indptr, indices, order, ptr = plan['indptr'], plan['indices'], plan['item_order'], plan['item_ptr']
    cand = np.empty((plan['nnz'], D), dtype=np.int32)
    for p in range(plan['nnz']):
        u, c = plan['users'][p], plan['item_part'][plan['items'][p]]
        seen, part = indices[indptr[u]:indptr[u + 1]], order[ptr[c]:ptr[c + 1]]
        for t in range(D):
            w = mix64((h + 64 * int(plan['perm'][p]) + t) & MASK) >> 32
            j = int(part[(w * len(part)) >> 32])
            at = int(np.searchsorted(seen, j))
            cand[p, t] = -1 if (at < len(seen) and seen[at] == j) else j
    return cand


# ---- the label embeddings -----------------------------------------------------------------------------------------------------
def label_image(feat, L):
    """S = F_lab L: per item (+0.0 + v1 * L[l1]) + v2 * L[l2] + ... in storage order"""
    n_items = len(feat['a'])
    S = np.zeros((n_items, L.shape[1]))
    for i in range(n_items):
        for e in range(feat['row_ptr'][i], feat['row_ptr'][i + 1]):
            S[i] = S[i] + feat['row_val'][e] * L[feat['row_idx'][e]]
    return S


def adagrad(x, A, g, lr):
    """in place: step = lr / sqrt(A); x <- x - step * g; A <- A + g * g"""
    step = lr / np.sqrt(A)
    x[...] = x - step * g
    A[...] = A + g * g


def label_step(feat, G, L, AL, lr):
    """g_l = (+0.0 + v1 * G[i1]) + v2 * G[i2] + ... over the label's items ascending; adagrad on L[l]; G is zeroed"""
    for l in range(feat['n_labels']):
        g = np.zeros(L.shape[1])
        for e in range(feat['col_ptr'][l], feat['col_ptr'][l + 1]):
            g = g + feat['col_val'][e] * G[feat['col_idx'][e]]
        adagrad(L[l], AL[l], g, lr)
    G[...] = 0.0


# ---- the epoch ----------------------------------------------------------------------------------------------------------------
def epoch(plan, cand, table, P, E, AP, AE, lr, feat=None, L=None, AL=None, trace=None):
    """one sweep in schedule order, everything updated in place; returns (trained, quiet, draws).  trace (a list) receives
    (position, violator's draw or -1) of every sample."""
    k = P.shape[1] - 1
    w = group_width(k + 1)
    B, bp, D = plan['blocks'], plan['block_ptr'], cand.shape[1]
    a = None if feat is None else feat['a']
    G = None if feat is None else np.zeros_like(E)
    trained = quiet = draws = 0
    for s in range(B):
        S = None if feat is None else label_image(feat, L)
        rep = (lambda j: E[j].copy()) if feat is None else (lambda j: a[j] * E[j] + S[j])
        for p in range(bp[s * B], bp[(s + 1) * B]):
            u, i = plan['users'][p], plan['items'][p]
            pu, qi = P[u].copy(), rep(i)
            x_pos = tree_sum(pu * qi, w)
            hit = -1
            for t in range(D):
                draws += 1
                j = cand[p, t]
                if j < 0:
                    continue
                qj = rep(j)
                x_neg = tree_sum(pu * qj, w)
                if not (x_neg > x_pos - 1.0):
                    continue
                lw = table[t]
                g_u, g_i, g_j = lw * (qj - qi), -lw * pu, lw * pu
                adagrad(P[u, :k], AP[u, :k], g_u[:k], lr)
                adagrad(E[i], AE[i], g_i if feat is None else a[i] * g_i, lr)
                adagrad(E[j], AE[j], g_j if feat is None else a[j] * g_j, lr)
                if feat is not None:
                    G[i] = G[i] + g_i
                    G[j] = G[j] + g_j
                trained += 1
                hit = t
                break
            if hit < 0:
                quiet += 1
            if trace is not None:
                trace.append((p, hit))
        if feat is not None:
            label_step(feat, G, L, AL, lr)
    return trained, quiet, draws


def representation(E, feat=None, L=None):
    """Q = a o E_id + F_lab E_lab (E itself without features)"""
    return E.copy() if feat is None else feat['a'][:, None] * E + label_image(feat, L)


def fit(dense, rank, learning_rate, max_sampled, num_epochs, seed, blocks, reshuffle_items=True, one_hot=None, init=None):
    """warp.warp_fit restated: dict of P, E, L (None without features), Q, the adagrad states, history (quiet share per epoch),
    trained / quiet / draws per epoch"""
    n_users, n_items = dense.shape
    feat = None if one_hot is None else make_features(one_hot)
    n_labels = 0 if feat is None else feat['n_labels']
    P, E, L = (x.copy() for x in (initial_embeddings(n_users, n_items, n_labels, rank, seed) if init is None else init))
    AP, AE, AL = np.ones_like(P), np.ones_like(E), np.ones_like(L)
    table = loss_table(n_items, max_sampled)
    out = dict(history=[], trained=[], quiet=[], draws=[])
    for ep in range(num_epochs):
        plan = make_plan(dense, blocks, item_order(seed, ep, n_items) if reshuffle_items else None)
        cand = draw_candidates(plan, seed, ep, max_sampled)
        t, q, d = epoch(plan, cand, table, P, E, AP, AE, learning_rate, feat, L, AL)
        out['history'].append(q / plan['nnz'] if plan['nnz'] else float('nan'))
        out['trained'].append(t), out['quiet'].append(q), out['draws'].append(d)
    out.update(P=P, E=E, L=L if feat is not None else None, Q=representation(E, feat, L), AP=AP, AE=AE, AL=AL, feat=feat)
    return out


def cold_queries(cold_one_hot, L):
    """(1 / m) sum of the label embeddings of a cold item's m known labels, storage order; an item without any gives zeros"""
    cold_one_hot = np.asarray(cold_one_hot) != 0
    out = np.zeros((cold_one_hot.shape[0], L.shape[1]))
    for i, row in enumerate(cold_one_hot):
        labels = np.flatnonzero(row)
        for l in labels:
            out[i] = out[i] + (1.0 / len(labels)) * L[l]
    return out


# ---- the naive loop -----------------------------------------------------------------------------------------------------------
def fold(d):
    if len(d) == 1:
        return d[0]
    h = len(d) // 2
    return fold([d[c] + d[c + h] for c in range(h)])


def naive_epoch(dense, order, blocks, max_sampled, seed, ep, P, E, AP, AE, lr, one_hot=None, L=None, AL=None):
    """the same epoch from the definitions: strata and blocks from the parts of users and items, entries from the dense rows,
    draws on the fly, Python floats one column at a time, features as dense loops.  Returns (trained, quiet, draws)."""
    n_users, n_items = dense.shape
    B, D, k = int(blocks), int(max_sampled), P.shape[1] - 1
    C = k + 1
    w = 16 if C <= 16 else 32 if C <= 32 else 64
    nnz = int(dense.sum())
    # parts: a user's (an ordered item's) part is floor(entries before it * B / nnz), at most B - 1
    upart, before = [], 0
    for u in range(n_users):
        upart.append(min(before * B // max(nnz, 1), B - 1))
        before += int(dense[u].sum())
    ipart, before = [0] * n_items, 0
    for i in order:
        ipart[i] = min(before * B // max(nnz, 1), B - 1)
        before += int(dense[:, i].sum())
    part_items = [[int(i) for i in order if ipart[i] == c] for c in range(B)]
    entry, e = {}, 0
    for u in range(n_users):
        for i in range(n_items):
            if dense[u, i]:
                entry[(u, i)] = e
                e += 1
    h = stream_key(seed, ep)
    # (NumPy's logarithm, as the specification says: libm's may round another way)
    table = [min(10.0, float(np.log(np.float64(max(1, (n_items - 1) // (t + 1)))))) for t in range(D)]
    feats = one_hot is not None
    if feats:
        hot = np.asarray(one_hot) != 0
        n_labels = hot.shape[1]
        a = [1.0 / (1.0 + int(hot[i].sum())) for i in range(n_items)]
        G = [[0.0] * C for _ in range(n_items)]
    trained = quiet = draws = 0

    def step(X, A, r, c, g):
        s = lr / math.sqrt(float(A[r, c]))
        X[r, c] = float(X[r, c]) - s * g
        A[r, c] = float(A[r, c]) + g * g

    for s in range(B):
        if feats:
            S = [[0.0] * C for _ in range(n_items)]
            for i in range(n_items):
                for l in range(n_labels):
                    if hot[i, l]:
                        for c in range(C):
                            S[i][c] = S[i][c] + a[i] * float(L[l, c])
        rep = (lambda j: [a[j] * float(E[j, c]) + S[j][c] for c in range(C)]) if feats else (lambda j: [float(v) for v in E[j]])
        for b in range(B):
            for u in range(n_users):
                if upart[u] != b:
                    continue
                for i in range(n_items):
                    if not dense[u, i] or (ipart[i] - b) % B != s:
                        continue
                    pu, qi = [float(v) for v in P[u]], rep(i)
                    x_pos = fold([pu[c] * qi[c] for c in range(C)] + [0.0] * (w - C))
                    part = part_items[ipart[i]]
                    hit = False
                    for t in range(D):
                        draws += 1
                        x = mix64((h + 64 * entry[(u, i)] + t) & MASK) >> 32
                        j = part[(x * len(part)) >> 32]
                        if dense[u, j]:
                            continue
                        qj = rep(j)
                        x_neg = fold([pu[c] * qj[c] for c in range(C)] + [0.0] * (w - C))
                        if not (x_neg > x_pos - 1.0):
                            continue
                        for c in range(C):
                            g_i, g_j = -table[t] * pu[c], table[t] * pu[c]
                            if c < k:
                                step(P, AP, u, c, table[t] * (qj[c] - qi[c]))
                            step(E, AE, i, c, a[i] * g_i if feats else g_i)
                            step(E, AE, j, c, a[j] * g_j if feats else g_j)
                            if feats:
                                G[i][c] = G[i][c] + g_i
                                G[j][c] = G[j][c] + g_j
                        trained += 1
                        hit = True
                        break
                    if not hit:
                        quiet += 1
        if feats:
            for l in range(n_labels):
                for c in range(C):
                    g = 0.0
                    for i in range(n_items):
                        if hot[i, l]:
                            g = g + a[i] * G[i][c]
                    step(L, AL, l, c, g)
            G = [[0.0] * C for _ in range(n_items)]
    return trained, quiet, draws


# ---- the CPU double of the WARP operators -------------------------------------------------------------------------------------
def numpy_ops():
    """NumpyOps plus what polara_amd/warp.py asks of HipOps (same semantics on CPU tensors)"""
    import torch
    from numpy_ops import NumpyOps

    class WarpNumpyOps(NumpyOps):
        def warp_max_rank(self):
            return MAX_RANK

        def warp_plan(self, A, blocks, item_order=None, features=None):
            dense = (A.m.toarray() != 0).astype(np.int8)
            plan = dict(make_plan(dense, blocks, item_order), matrix=A, features=None)
            if features is not None:
                plan['features'] = make_features(features.toarray())
            return plan

        def warp_draw(self, plan, seed, epoch, max_sampled):
            return torch.from_numpy(draw_candidates(plan, seed, epoch, max_sampled))

        def warp_label_image(self, plan, L):
            return torch.from_numpy(label_image(plan['features'], L.numpy()))

        def warp_representation(self, plan, E, L=None):
            return torch.from_numpy(representation(E.numpy(), plan['features'], None if L is None else L.numpy()))

        def warp_epoch(self, plan, cand, table, P, E, state, learning_rate, L=None):
            AP, AE, AL = state
            feat = plan['features']
            return torch.tensor(epoch(plan, cand.numpy(), np.asarray(table), P.numpy(), E.numpy(), AP.numpy(), AE.numpy(),
                                      float(learning_rate), feat, None if feat is None else L.numpy(),
                                      None if feat is None else AL.numpy()), dtype=torch.int64)

    return WarpNumpyOps()


# ---- test matrices ------------------------------------------------------------------------------------------------------------
def random_features(n_items=23, n_labels=6, seed=1):
    """0/1 [n_items x n_labels]: about two labels per item, item 0 with none, label 0 on every other item; with any
    non-trivial item order the items of a label fall into different parts"""
    hot = (np.random.RandomState(seed).rand(n_items, n_labels) < 0.3).astype(np.int8)
    hot[:, 0] = 1
    hot[0] = 0
    return hot


def planted_cold_start(seed=5, n_users=60, n_warm=40, n_cold=8, p_in=0.45, p_out=0.05, n_noise=6):
    """(train [n_users x n_warm], holdout item per user, one-hot of the warm items, cold likes [n_users x n_cold], one-hot of
    the cold items): two user groups x two item groups of equal expected popularity; every item carries its group's label
    (0 or 1) and one of `n_noise` noise labels; one positive per user is held out of the warm block"""
    rng = np.random.RandomState(seed)
    n_items = n_warm + n_cold
    ug = np.arange(n_users) * 2 // n_users
    ig = np.concatenate([np.arange(n_warm) * 2 // n_warm, np.arange(n_cold) * 2 // n_cold])
    likes = (rng.rand(n_users, n_items) < np.where(ug[:, None] == ig[None, :], p_in, p_out)).astype(np.int8)
    hot = np.zeros((n_items, 2 + n_noise), dtype=np.int8)
    hot[np.arange(n_items), ig] = 1
    hot[np.arange(n_items), 2 + rng.randint(n_noise, size=n_items)] = 1
    train = likes[:, :n_warm].copy()
    holdout = np.empty(n_users, dtype=np.int64)
    for u in range(n_users):
        liked = np.flatnonzero(train[u])
        assert len(liked) >= 2
        holdout[u] = liked[rng.randint(len(liked))]
        train[u, holdout[u]] = 0
    return train, holdout, hot[:n_warm], likes[:, n_warm:], hot[n_warm:]


def cold_auc(scores, cold_likes):
    """mean over cold items (with at least one fan and one other user) of the share of (fan, other) pairs ranked right;
    scores [n_cold x n_users], ties count half"""
    total, n = 0.0, 0
    for c in range(scores.shape[0]):
        fans, rest = np.flatnonzero(cold_likes[:, c] > 0), np.flatnonzero(cold_likes[:, c] == 0)
        if len(fans) == 0 or len(rest) == 0:
            continue
        d = scores[c, fans][:, None] - scores[c, rest][None, :]
        total += ((d > 0).sum() + 0.5 * (d == 0).sum()) / d.size
        n += 1
    return total / n
