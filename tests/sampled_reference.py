"""NumPy restatements of the sampled-evaluation operators (csrc/sampled.hip), the references of tests/test_gpu_sampled.py
and the CPU double of tests/test_dropin_sampled.py:

  * `gathered_scores`: s[u, c] = sum_f P[u, f] * V[cand[u, c], f], f ascending from +0.0, every product and every sum a
    separate NumPy operation (separately rounded: no fused multiply-add) — the loop of the reference's `inner_product_at`
    (lib/sparse.py:66-71) and `mf_random_item_scoring` (lib/sampler.py:88-93);
  * `select`: the first k column positions by (score descending, position ascending), -0 equal to +0, NaN last;
  * `sample_unseen`: the sampler's definition, draw by draw."""
import numpy as np

MASK64 = (1 << 64) - 1


def gathered_scores(P, V, cand):
    P, V, cand = np.asarray(P, dtype=np.float64), np.asarray(V, dtype=np.float64), np.asarray(cand, dtype=np.int64)
    s = np.zeros(cand.shape, dtype=np.float64)
    for f in range(P.shape[1]):
        prod = P[:, f][:, None] * V[cand, f]
        s = s + prod
    return s


def select(scores, topk):
    t = np.array(scores, dtype=np.float64)
    t[np.isnan(t)] = -np.inf
    return np.argsort(-t, axis=1, kind='stable')[:, :int(topk)].astype(np.int64)


def candidates_topk(P, V, cand, topk):
    scores = gathered_scores(P, V, cand)
    return select(scores, topk), scores


def mix64(z):
    """the splitmix64 output function on a Python int"""
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed, t, n_items):
    """draw t of the user with this seed: an item id, or None when the draw is rejected by the unbiased mapping"""
    w = mix64(((int(seed) & 0xffffffff) << 32) | int(t)) >> 32
    m = w * int(n_items)
    if (m & 0xffffffff) < (1 << 32) % int(n_items):
        return None
    return m >> 32


def sample_unseen_row(seed, n_items, excluded, n):
    excluded = set(int(x) for x in excluded)
    if n > n_items - len(excluded):
        raise ValueError('%d items wanted, %d eligible' % (n, n_items - len(excluded)))
    out, taken, t = [], set(), 0
    while len(out) < n:
        x = draw(seed, t, n_items)
        t += 1
        if x is None or x in excluded or x in taken:
            continue
        taken.add(x)
        out.append(x)
    return out


def sample_unseen(t_indptr, t_indices, h_indptr, h_indices, n_items, n, seeds):
    """int32 [n_users x n]: rows of two CSR structures excluded (the second may be None)"""
    n_users = len(t_indptr) - 1
    out = np.empty((n_users, int(n)), dtype=np.int32)
    for u in range(n_users):
        ex = list(t_indices[t_indptr[u]:t_indptr[u + 1]])
        if h_indptr is not None:
            ex += list(h_indices[h_indptr[u]:h_indptr[u + 1]])
        out[u] = sample_unseen_row(seeds[u], n_items, ex, n)
    return out
