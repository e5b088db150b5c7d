"""numpy restatement of the settle tier of the first re-scoring (csrc/rescore.hip, rescore_topk_kernel) and the test cases
built around it: CPU code, no device.

The rule.  The candidate sweep scores item i for user u as s32 with |s32 - E'_u . V_i| <= B ||E'_u|| ||V_i||,
B = 3 * 2^-16 + (4 K + 10) * 2^-23, and the rows E' it works on are an approximate fold-in: ||E'_u - E_u|| <= 2^-24 w_u.  With
N_u >= ||E'_u||, n_i >= ||V_i|| and a_u = 2^-24 w_u (1 + 1e-6), every sweep score is within d_i = (B N_u + a_u) n_i of the exact
score of the same item.  A user's candidates sorted by sweep score (descending, item ascending) are in their exact order, and
their first topk are the exact top-k, when
    s_t - s_{t+1} > d_t + d_{t+1}          for t = 1 .. topk,
    s_topk - s_j  > d_topk + d_j           for every later entry j,
    s_topk - tau_cert > d_topk + d_max     when a list was full (tau32 = its last entry, tau_cert = tau32 + |tau32| 2^-15,
                                           d_max = d at n = vmax): items the sweep left out,
and the user has at least topk unseen items and no unbounded list.  Such a user is settled."""
import numpy as np

IDX_NONE = 0x7fffffff


def sweep_err_coeff(K):
    return 3.0 * 2.0 ** -16 + (4 * K + 10) * 2.0 ** -23


def settle(cand_score, cand_idx, KC, splits, n_users, topk, K, user_norm, e_err, item_norm, vmax, n_items, n_seen):
    """cand_score (float32) / cand_idx (int32): the sweep's lists, [splits][n_pad][KC]; user_norm float32 [n_users]; e_err
    float64 [n_users] (w_u); item_norm float32 [n_items] or None.  Returns (settled bool [n_users], margin float64 [n_users]):
    margin = the smallest (gap - bound) / bound over the user's conditions (> 0: settled; within 1e-6 of 0: the device's
    rounding of the same expressions may decide either way)."""
    n_pad = -(-n_users // 32) * 32
    cs = np.asarray(cand_score, dtype=np.float32).reshape(splits, n_pad, KC).astype(np.float64)
    ci = np.asarray(cand_idx, dtype=np.int32).reshape(splits, n_pad, KC)
    B = sweep_err_coeff(K)
    settled = np.zeros(n_users, dtype=bool)
    margin = np.full(n_users, -np.inf)
    for u in range(n_users):
        s = cs[:, u, :].reshape(-1)
        i = ci[:, u, :].reshape(-1)
        last = ci[:, u, KC - 1]
        unbounded = bool((last == -2).any())
        full = last >= 0
        tau32 = cs[full, u, KC - 1].max() if full.any() else -np.inf
        ok = i >= 0
        s, i = s[ok], i[ok].astype(np.int64)
        order = np.lexsort((i, -s))
        s, i = s[order], i[order]
        if unbounded or n_items - n_seen[u] < topk or len(s) < topk:
            continue
        c = B * float(user_norm[u]) + float(e_err[u]) * 2.0 ** -24 * (1.0 + 1e-6)
        d_max = c * vmax
        d = np.full(len(s), d_max) if item_norm is None else c * np.minimum(vmax, item_norm[i].astype(np.float64) * (1.0 + 1e-6))
        # entries behind the end of the list: -inf at d_max
        s = np.append(s, -np.inf)
        d = np.append(d, d_max)
        gaps, bounds = [], []
        for t in range(topk):
            gaps.append(s[t] - s[t + 1])
            bounds.append(d[t] + d[t + 1])
        for j in range(topk, len(s)):
            gaps.append(s[topk - 1] - s[j])
            bounds.append(d[topk - 1] + d[j])
        if tau32 > -np.inf:
            gaps.append(s[topk - 1] - (tau32 + abs(tau32) * 2.0 ** -15))
            bounds.append(d[topk - 1] + d_max)
        gaps, bounds = np.array(gaps), np.array(bounds)
        with np.errstate(invalid='ignore', divide='ignore'):
            settled[u] = bool(np.all(gaps > bounds))
            margin[u] = np.min(np.where(bounds > 0, (gaps - bounds) / bounds, np.where(gaps > bounds, np.inf, -np.inf)))
    return settled, margin


def exact_stand_in(V, E, indptr, indices, KC, w, extra_scale=1.2e-7):
    """The inputs of `settle` with exact fp64 scores standing in for the sweep's (one split, the KC best unseen items per user):
    what the rule does on a case can be seen on the CPU before any device run.  w: the fold-in's error weights."""
    n_users, n_items = E.shape[0], V.shape[0]
    n_pad = -(-n_users // 32) * 32
    cs = np.full((1, n_pad, KC), -np.inf, dtype=np.float32)
    ci = np.full((1, n_pad, KC), -1, dtype=np.int32)
    S = E @ V.T
    for u in range(n_users):
        s = S[u].copy()
        s[indices[indptr[u]:indptr[u + 1]]] = -np.inf
        order = np.lexsort((np.arange(n_items), -s))[:KC]
        order = order[np.isfinite(s[order])]
        cs[0, u, :len(order)] = s[order]
        ci[0, u, :len(order)] = order
    vnorm = (np.linalg.norm(V, axis=1) * (1 + 1e-6)).astype(np.float32)
    un = (np.linalg.norm(E, axis=1) * (1 + 1e-6) + extra_scale * w).astype(np.float32)
    return cs, ci, un, vnorm, float(vnorm.max())


def brute_topk(V, E, indptr, indices, topk, same=()):
    """the reference order: unseen items first, score descending (fp64), item ascending; `same`: pairs (i, j) of identical item
    rows, whose scores are made the same bits whatever the matrix product did with them"""
    S = E @ V.T
    for i, j in same:
        S[:, j] = S[:, i]
    n_users, n_items = S.shape
    out = np.empty((n_users, topk), dtype=np.int64)
    for u in range(n_users):
        cls = np.zeros(n_items, dtype=np.int64)
        cls[indices[indptr[u]:indptr[u + 1]]] = 1
        out[u] = np.lexsort((np.arange(n_items), -S[u], cls))[:topk]
    return out


def random_csr(rng, n_users, n_items, lo, hi, p=None):
    """non-negative feedback (the approximate fold-in needs it), lo..hi entries per row drawn with item probabilities p"""
    indptr, idx, val = [0], [], []
    for _ in range(n_users):
        n = int(rng.randint(lo, hi + 1))
        cols = np.sort(rng.choice(n_items, size=n, replace=False, p=p))
        idx.append(cols)
        val.append(rng.randint(1, 6, size=n).astype(np.float32))
        indptr.append(indptr[-1] + n)
    return np.asarray(indptr, dtype=np.int64), np.concatenate(idx).astype(np.int32), np.concatenate(val)


def fold(indptr, indices, values, V):
    E = np.zeros((len(indptr) - 1, V.shape[1]))
    for u in range(len(indptr) - 1):
        sl = slice(indptr[u], indptr[u + 1])
        E[u] = values[sl].astype(np.float64) @ V[indices[sl]]
    return E


def fold_weights(indptr, indices, values, V, scale=40.0):
    """a stand-in for the fold-in's error weights on the CPU: sum_j a_uj ||V_j||, times what the packed image costs (~40)"""
    vn = np.linalg.norm(V, axis=1)
    return scale * np.array([float(values[indptr[u]:indptr[u + 1]].astype(np.float64) @ vn[indices[indptr[u]:indptr[u + 1]]])
                             for u in range(len(indptr) - 1)])


def decaying_catalogue(seed, n_items, K, latent=3, noise=2e-3, decay=0.5, clones=0, cone=0.0):
    """item factors of a low-rank catalogue with decaying row norms: `latent` directions carry the rows, a little noise in
    the others — the items of one direction score close to each other, so a share of the users has top-k gaps inside the
    sweep's error bound and a share has not.  cone > 0: every row has a component of at least `cone` along the first
    direction — all scores of a user with non-negative feedback are positive (and all negative once its row is negated)"""
    rng = np.random.RandomState(seed)
    Z = rng.randn(n_items, latent)
    if cone > 0.0:
        Z[:, 0] = cone + np.abs(Z[:, 0])
    W = np.linalg.qr(rng.randn(K, latent))[0].T
    V = Z @ W + noise * rng.randn(n_items, K)
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    V *= ((1.0 + np.arange(n_items)) ** -decay)[:, None]
    # `clones` popular items get a neighbour 3e-5 (relative) shorter: whoever ranks such a pair in its top-k cannot settle
    for j in rng.choice(np.arange(0, min(n_items, 240) - 1, 2), size=clones, replace=False):
        V[j + 1] = V[j] * (1.0 - 3e-5)
    return V


def flat_catalogue(seed, n_items, K):
    rng = np.random.RandomState(seed)
    V = rng.randn(n_items, K)
    return V / np.linalg.norm(V, axis=1, keepdims=True)


def popularity(n_items):
    p = (1.0 + np.arange(n_items)) ** -0.7
    return p / p.sum()
