"""TEST-ONLY NumPy restatement of contextual post-filtering, written from the formulas (not from the kernel):

  * the LITERAL arithmetic of the reference (contextual/models.py:5-32 followed by models.py:359-371): per chunk of users and
    per context in order, M = max of the chunk, every (user, item of the user's value) becomes M + s + 1; then the seen items
    are down-voted and the top-k taken;
  * the CLASS order of the contract: class = sum_j 2^j [item in the list of the user's value of context j] over the unseen
    items, then score descending, then item ascending; seen items are never up-voted and follow, when a row runs out of
    unseen items, in the order of the plain pass;
  * `merge_reference`: what pk_context_merge_f64 returns for given base lists, and a `NumpyOps` subclass that serves it, so
    that the model layer runs in the GPU-less container.
"""
import numpy as np
import torch

from numpy_ops import NumpyOps
from polara_amd import contextual


def user_lists(contexts, u):
    """the item list of user u in every context: contexts = [(user_value, value_ptr, value_items), ...]"""
    out = []
    for uv, ptr, items in contexts:
        v = int(uv[u])
        out.append(np.asarray(items[ptr[v]:ptr[v + 1]], dtype=np.int64) if v >= 0 else np.zeros(0, dtype=np.int64))
    return out


def classes(contexts, n_users, n_items):
    """int64 [n_users x n_items]: the class of every (user, item)"""
    cls = np.zeros((n_users, n_items), dtype=np.int64)
    for u in range(n_users):
        for j, lst in enumerate(user_lists(contexts, u)):
            cls[u, lst] |= 1 << j
    return cls


def seen_mask(seen_ptr, seen_idx, n_users, n_items):
    m = np.zeros((n_users, n_items), dtype=bool)
    if seen_ptr is not None:
        for u in range(n_users):
            m[u, seen_idx[seen_ptr[u]:seen_ptr[u + 1]]] = True
    return m


def topk_desc(scores, topk):
    """score descending, item ascending"""
    n = scores.shape[1]
    return np.stack([np.lexsort((np.arange(n), -row))[:topk] for row in scores])


def literal_lists(scores, contexts, seen, topk, chunk=None):
    """the reference's own arithmetic: up-vote per chunk, down-vote the seen items (models.py:494-519), top-k"""
    n_users, n_items = scores.shape
    chunk = chunk or n_users
    out = np.empty((n_users, topk), dtype=np.int64)
    for s0 in range(0, n_users, chunk):
        s1 = min(n_users, s0 + chunk)
        block = scores[s0:s1].copy()
        for j in range(len(contexts)):
            rows, cols = [], []
            for u in range(s0, s1):
                lst = user_lists(contexts, u)[j]
                rows.append(np.full(len(lst), u - s0))
                cols.append(lst)
            rows, cols = np.concatenate(rows), np.concatenate(cols)
            block[rows, cols] = block.max() + block[rows, cols] + 1
        sm = seen[s0:s1]
        if sm.any():
            sv = block[sm]
            block[sm] = block.min() - (sv.max() - sv) - 1
        out[s0:s1] = topk_desc(block, topk)
    return out


def class_order_lists(scores, contexts, seen, topk):
    """(ids, classes) of the contract: unseen items by (class desc, score desc, item asc), then the seen tail in the order of
    the plain pass (score desc, item asc), class 0"""
    n_users, n_items = scores.shape
    cls = np.where(seen, 0, classes(contexts, n_users, n_items))
    ids = np.empty((n_users, topk), dtype=np.int64)
    for u in range(n_users):
        ids[u] = np.lexsort((np.arange(n_items), -scores[u], -cls[u], seen[u]))[:topk]
    return ids, np.take_along_axis(cls, ids, 1).astype(np.int32)


def plain_lists(scores, seen, topk):
    """the lists of the plain pass: unseen by (score desc, item asc), then the seen tail"""
    n = scores.shape[1]
    return np.stack([np.lexsort((np.arange(n), -scores[u], seen[u]))[:topk] for u in range(scores.shape[0])])


def min_gap(scores, seen, topk):
    """the smallest distance between neighbouring scores over ranks 1..topk+1 of the unseen items of any user: when it is
    far above the rounding of a K-term fp64 dot product, every summation order gives the same lists"""
    s = np.where(seen, -np.inf, scores)
    head = -np.sort(-s, axis=1)[:, :topk + 1]
    d = head[:, :-1] - head[:, 1:]
    return float(d[np.isfinite(d)].min())


def class_order_gap(scores, contexts, seen, topk):
    """the smallest distance between neighbouring scores of ONE class over ranks 1..topk+1 of the class order of any user:
    context items far down the plain ranking are neighbours in the tier, so the plain gap alone does not cover them"""
    n_users, n_items = scores.shape
    cls = np.where(seen, 0, classes(contexts, n_users, n_items))
    best = np.inf
    for u in range(n_users):
        head = np.lexsort((np.arange(n_items), -scores[u], -cls[u], seen[u]))[:topk + 1]
        same = (cls[u, head[:-1]] == cls[u, head[1:]]) & (seen[u, head[:-1]] == seen[u, head[1:]])
        d = (scores[u, head[:-1]] - scores[u, head[1:]])[same]
        if len(d):
            best = min(best, float(d.min()))
    return best


def merge_reference(V, E, seen_ptr, seen_idx, contexts, base_idx, scores=None):
    """(out_idx, out_class) of pk_context_merge_f64 from its contract: the best topk unseen context items of the user under
    (class desc, score desc, item asc), then the base entries that are not among the user's unseen context items, in their
    order, up to topk; pads (-1) stay at the end"""
    n_users, topk = base_idx.shape
    n_items = V.shape[0]
    scores = E @ V.T if scores is None else scores
    out = np.full((n_users, topk), -1, dtype=np.int64)
    out_cls = np.zeros((n_users, topk), dtype=np.int32)
    for u in range(n_users):
        cls = np.zeros(n_items, dtype=np.int64)
        for j, lst in enumerate(user_lists(contexts, u)):
            cls[lst] |= 1 << j
        if seen_ptr is not None:
            cls[seen_idx[seen_ptr[u]:seen_ptr[u + 1]]] = 0
        tier = np.flatnonzero(cls)
        tier = tier[np.lexsort((tier, -scores[u, tier], -cls[tier]))][:topk]
        rest = [b for b in base_idx[u] if b < 0 or cls[b] == 0][:topk - len(tier)]
        out[u, :len(tier)] = tier
        out_cls[u, :len(tier)] = cls[tier]
        out[u, len(tier):len(tier) + len(rest)] = rest
    return out, out_cls


class ContextNumpyOps(NumpyOps):
    """NumpyOps plus the two contextual methods of HipOps"""

    def context_lists(self, user_value, value_ptr, value_items, n_users, n_items):
        uv, ptr, items, max_list = contextual.check_context_lists(user_value, value_ptr, value_items, n_users, n_items)
        return contextual.ContextLists(torch.from_numpy(uv), torch.from_numpy(ptr), torch.from_numpy(items), max_list)

    def context_merge(self, V, E, seen, contexts, base_idx, want_class=False, order=None):
        sp, si = (None, None) if seen is None else (seen[0].numpy(), seen[1].numpy())
        if order is not None:
            assert sorted(order.tolist()) == list(range(base_idx.shape[0]))
        ctx = [(c.user_value.numpy(), c.value_ptr.numpy(), c.value_items.numpy()) for c in contexts]
        out, cls = merge_reference(V.numpy(), E.numpy(), sp, si, ctx, base_idx.numpy())
        return torch.from_numpy(out), (torch.from_numpy(cls) if want_class else None)


def construction(n_users=192, n_items=5000, K=16, n_seen=20, sizes_a=(0, 1, 3, 40, 4500, 7), sizes_b=(0, 12, 600), seed=0,
                 gaussian=False):
    """The construction of the issue's check: non-negative rank-K factors (or Gaussian x 3: scores below -1), n_seen seen items
    per user, two contexts with the given value-list sizes; some users have no value in context b.
    -> (V, E, seen_ptr, seen_idx, [(user_value, ptr, items) x 2])"""
    rng = np.random.RandomState(seed)
    if gaussian:
        V, E = 3 * rng.randn(n_items, K), 3 * rng.randn(n_users, K)
    else:
        V, E = rng.rand(n_items, K), rng.rand(n_users, K)
    seen_idx = np.concatenate([np.sort(rng.choice(n_items, n_seen, replace=False)) for _ in range(n_users)]).astype(np.int32)
    seen_ptr = np.arange(n_users + 1, dtype=np.int64) * n_seen
    contexts = []
    for sizes, with_none in ((sizes_a, False), (sizes_b, True)):
        lists = [np.sort(rng.choice(n_items, s, replace=False)) for s in sizes]
        ptr = np.r_[0, np.cumsum([len(l) for l in lists])].astype(np.int64)
        items = (np.concatenate(lists) if len(lists) else np.zeros(0)).astype(np.int32)
        uv = rng.randint(-1 if with_none else 0, len(sizes), n_users).astype(np.int32)
        uv[:len(sizes)] = np.arange(len(sizes))           # every value occurs
        contexts.append((uv, ptr, items))
    return V, E, seen_ptr, seen_idx, contexts
