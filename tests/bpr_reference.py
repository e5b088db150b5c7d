"""TEST-ONLY NumPy restatement of BPR (polara_amd/bpr.py, csrc/bpr.hip; the specification is the comment in
include/polara_hip.h): the item order, the schedule, the draws, the sigmoid and the epoch, sample by sample in schedule order —
a blocked epoch IS the serial sweep on the scheduled list, because the blocks of a stratum share no row.  Never imported by the
package.

Below it, `naive_epoch`: a second, deliberately naive LearnBPR loop for B = 1 straight over the CSR rows with Python floats.  It
shares nothing with the restatement but `sigmoid` and `draw`."""
import numpy as np

MAX_RANK = 63
DRAWS = 4
MASK = (1 << 64) - 1

EXP_MIN = -750.0
LOG2E = float.fromhex('0x1.71547652b82fep+0')
LN2_HI = float.fromhex('0x1.62e42fee00000p-1')
LN2_LO = float.fromhex('0x1.a39ef35793c76p-33')
TAYLOR = [float.fromhex(h) for h in (                   # 1 / 13!, 1 / 12!, .. 1 / 2!, then 1, 1
    '0x1.6124613a86d09p-33', '0x1.1eed8eff8d898p-29', '0x1.ae64567f544e4p-26', '0x1.27e4fb7789f5cp-22', '0x1.71de3a556c734p-19',
    '0x1.a01a01a01a01ap-16', '0x1.a01a01a01a01ap-13', '0x1.6c16c16c16c17p-10', '0x1.1111111111111p-7', '0x1.5555555555555p-5',
    '0x1.5555555555555p-3', '0x1.0000000000000p-1', '0x1p+0', '0x1p+0')]


def sigmoid(x):
    """1 / (1 + exp(x)) elementwise, by the device's sequence of IEEE operations (+ - * /, floor, comparisons, ldexp)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid='ignore', under='ignore'):
        pos = x > 0.0
        a = np.where(pos, -x, x)
        a = np.where(a < EXP_MIN, EXP_MIN, a)
        n = np.floor(a * LOG2E + 0.5)
        r = (a - n * LN2_HI) - n * LN2_LO
        p = np.full_like(x, TAYLOR[0])
        for c in TAYLOR[1:]:
            p = p * r + c
        e = np.ldexp(p, np.where(n == n, n, 0.0).astype(np.int64))
        return np.where(pos, e, 1.0) / (1.0 + e)


def mix64(z):
    """the splitmix64 output function on a Python int, modulo 2**64"""
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def stream_key(seed, epoch):
    return mix64(((int(seed) << 32) + int(epoch)) & MASK)


def draw(h, e, seen, part_items):
    """the negative of canonical entry e: the first of DRAWS draws from `part_items` that is not in the sorted row `seen`, or -1"""
    n_c = len(part_items)
    for t in range(DRAWS):
        w = mix64((h + 4 * int(e) + t) & MASK) >> 32
        j = int(part_items[(w * n_c) >> 32])
        at = int(np.searchsorted(seen, j))
        if not (at < len(seen) and seen[at] == j):
            return j
    return -1


def item_order(seed, epoch, n_items):
    return np.random.RandomState(np.array([int(seed), int(epoch)], dtype=np.uint32)).permutation(int(n_items)).astype(np.int64)


def parts(counts, blocks, nnz):
    counts = np.asarray(counts, dtype=np.int64)
    return np.minimum((np.cumsum(counts) - counts) * blocks // max(int(nnz), 1), blocks - 1)


def canonical(dense):
    """(indptr int64, indices int32, users int64, items int64) of the non-zeros of a dense 0/1 array: the canonical CSR"""
    users, items = np.nonzero(dense)
    indptr = np.zeros(dense.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(users, minlength=dense.shape[0]), out=indptr[1:])
    return indptr, items.astype(np.int32), users.astype(np.int64), items.astype(np.int64)


def make_plan(dense, blocks, order=None):
    """the plan dict of HipOps.bpr_plan as NumPy arrays (plus the CSR) from a dense 0/1 array"""
    n_users, n_items = dense.shape
    indptr, indices, users, items = canonical(dense)
    B, nnz = int(blocks), len(users)
    order = np.arange(n_items, dtype=np.int64) if order is None else np.asarray(order, dtype=np.int64)
    upart = parts(np.bincount(users, minlength=n_users), B, nnz)
    ordered = parts(np.bincount(items, minlength=n_items)[order], B, nnz)
    ipart = np.empty(n_items, dtype=np.int64)
    ipart[order] = ordered
    item_ptr = np.concatenate([[0], np.cumsum(np.bincount(ordered, minlength=B))]).astype(np.int64)
    key = ((ipart[items] - upart[users]) % B) * B + upart[users]
    perm = np.argsort(key, kind='stable').astype(np.int64)
    block_ptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=B * B))]).astype(np.int64)
    return dict(blocks=B, nnz=nnz, shape=(n_users, n_items), perm=perm, block_ptr=block_ptr, item_ptr=item_ptr,
                users=users[perm].astype(np.int32), items=items[perm].astype(np.int32), item_order=order.astype(np.int32),
                item_part=ipart.astype(np.int32), indptr=indptr, indices=indices)


def draw_negatives(plan, seed, epoch):
    """int32 [nnz]: the negative of every position of the schedule, -1: skipped"""
    h = stream_key(seed, epoch)
    indptr, indices, order, ptr = plan['indptr'], plan['indices'], plan['item_order'], plan['item_ptr']
    neg = np.empty(plan['nnz'], dtype=np.int32)
    for p in range(plan['nnz']):
        u, c = plan['users'][p], plan['item_part'][plan['items'][p]]
        neg[p] = draw(h, plan['perm'][p], indices[indptr[u]:indptr[u + 1]], order[ptr[c]:ptr[c + 1]])
    return neg


def group_width(columns):
    return 16 if columns <= 16 else 32 if columns <= 32 else 64


def tree_sum(v, w):
    d = np.zeros(w)
    d[:len(v)] = v
    h = w // 2
    while h >= 1:
        d = d[:h] + d[h:2 * h]
        h //= 2
    return d[0]


def epoch(plan, neg, P, Q, lr, reg):
    """one sweep in schedule order, P and Q [.. x (k + 1)] updated in place; returns (trained, skipped, correct)"""
    k = P.shape[1] - 1
    w = group_width(k + 1)
    trained = skipped = correct = 0
    for p in range(plan['nnz']):
        u, i, j = plan['users'][p], plan['items'][p], neg[p]
        if j < 0:
            skipped += 1
            continue
        pu, qi, qj = P[u].copy(), Q[i].copy(), Q[j].copy()
        d = qi - qj
        x = tree_sum(pu * d, w)
        z = float(sigmoid(x))
        P[u, :k] = (pu + lr * (z * d - reg * pu))[:k]
        Q[i] = qi + lr * (z * pu - reg * qi)
        Q[j] = qj - lr * (z * pu + reg * qj)
        correct += int(x > 0)
        trained += 1
    return trained, skipped, correct


def initial_factors(n_users, n_items, rank, seed):
    rnds = np.random.RandomState(seed)
    P0, Q0 = np.ones((n_users, rank + 1)), np.zeros((n_items, rank + 1))
    P0[:, :rank] = (rnds.rand(n_users, rank) - 0.5) / rank
    Q0[:, :rank] = (rnds.rand(n_items, rank) - 0.5) / rank
    return P0, Q0


def fit(dense, rank, learning_rate, regularization, num_epochs, seed, blocks, reshuffle_items=True, init=None):
    """bpr.bpr_fit restated: (P, Q, auc_history, skipped per epoch)"""
    n_users, n_items = dense.shape
    P, Q = (a.copy() for a in (initial_factors(n_users, n_items, rank, seed) if init is None else init))
    auc, skipped = [], []
    for ep in range(num_epochs):
        plan = make_plan(dense, blocks, item_order(seed, ep, n_items) if reshuffle_items else None)
        t, s, c = epoch(plan, draw_negatives(plan, seed, ep), P, Q, learning_rate, regularization)
        auc.append(c / t if t else float('nan'))
        skipped.append(s)
    return P, Q, auc, skipped


# ---- the naive loop (B = 1) --------------------------------------------------------------------------------------------------
def fold(d):
    if len(d) == 1:
        return d[0]
    h = len(d) // 2
    return fold([d[c] + d[c + h] for c in range(h)])


def naive_epoch(dense, order, P, Q, lr, reg, seed, ep):
    """LearnBPR over the rows of `dense`, user after user, item after item, negatives from the whole catalogue in the order
    `order`; Python floats, one column at a time.  Returns (trained, skipped, correct)."""
    n_users, n_items = dense.shape
    k = P.shape[1] - 1
    w = 16 if k < 16 else 32 if k < 32 else 64
    h = stream_key(seed, ep)
    e = trained = skipped = correct = 0
    for u in range(n_users):
        seen = np.flatnonzero(dense[u])
        for i in seen:
            j = draw(h, e, seen, order)
            e += 1
            if j < 0:
                skipped += 1
                continue
            pu, qi, qj = [float(v) for v in P[u]], [float(v) for v in Q[i]], [float(v) for v in Q[j]]
            x = fold([pu[c] * (qi[c] - qj[c]) for c in range(k + 1)] + [0.0] * (w - k - 1))
            z = float(sigmoid(x))
            for c in range(k + 1):
                dc = qi[c] - qj[c]
                if c < k:
                    P[u, c] = pu[c] + lr * (z * dc - reg * pu[c])
                Q[i, c] = qi[c] + lr * (z * pu[c] - reg * qi[c])
                Q[j, c] = qj[c] - lr * (z * pu[c] + reg * qj[c])
            if x > 0:
                correct += 1
            trained += 1
    return trained, skipped, correct


# ---- the CPU double of the BPR operators -------------------------------------------------------------------------------------
def numpy_ops():
    """NumpyOps plus what polara_amd/bpr.py asks of HipOps (same semantics on CPU tensors)"""
    import torch
    from numpy_ops import NumpyOps

    class BPRNumpyOps(NumpyOps):
        def bpr_max_rank(self):
            return MAX_RANK

        def bpr_plan(self, A, blocks, item_order=None):
            dense = (A.m.toarray() != 0).astype(np.int8)
            return dict(make_plan(dense, blocks, item_order), matrix=A)

        def bpr_draw_negatives(self, plan, seed, epoch):
            return torch.from_numpy(draw_negatives(plan, seed, epoch))

        def bpr_epoch(self, plan, neg, P, Q, learning_rate, regularization):
            if int(P.shape[1]) - 1 > MAX_RANK:
                raise ValueError('BPR: rank %d outside 1..%d' % (P.shape[1] - 1, MAX_RANK))
            return torch.tensor(epoch(plan, neg.numpy(), P.numpy(), Q.numpy(), float(learning_rate), float(regularization)),
                                dtype=torch.int64)

    return BPRNumpyOps()


# ---- test matrices --------------------------------------------------------------------------------------------------------------
def random_matrix(n_users=37, n_items=23, density=0.3, seed=0):
    return (np.random.RandomState(seed).rand(n_users, n_items) < density).astype(np.int8)


def corner_matrix():
    """(8 users x 6 items, an item order): item 0 is liked by everybody and user 0 likes every other item.  With B = 2 along
    the order (non-identity, item 0 first) item 0 is a part of its own — all its positives are skipped — and user 0 has seen
    the whole other part — all their positives there are skipped"""
    dense = np.zeros((8, 6), dtype=np.int8)
    dense[:, 0] = 1
    dense[0, 1:] = 1
    dense[1, 1] = dense[2, 2] = 1
    return dense, np.array([0, 5, 4, 3, 2, 1], dtype=np.int64)


def forwarding_matrix():
    """5 users x 3 items, one part (B = 1).  The sweep's samples are (0, 0), (0, 1), (1, 2), (2, 0), (3, 1), (4, 1): a user with
    two positives, whose negatives are both item 2; then the positive 2; with the right seed (`FORWARDING_SEED`) samples 2 and 3
    are (1, 2, 0) and (2, 0, 2) — each one's negative is the other's positive —; the last two share their positive"""
    dense = np.zeros((5, 3), dtype=np.int8)
    dense[0, 0] = dense[0, 1] = dense[1, 2] = dense[2, 0] = dense[3, 1] = dense[4, 1] = 1
    return dense


def planted_matrix(seed=3, n_users=60, n_items=40, p_in=0.5, p_out=0.05):
    """(train, holdout item per user): two user groups x two item groups of equal size and equal expected item popularity —
    a user likes an item of its own group with probability p_in, of the other with p_out — and one positive per user held out"""
    rng = np.random.RandomState(seed)
    ug, ig = np.arange(n_users) * 2 // n_users, np.arange(n_items) * 2 // n_items
    dense = (rng.rand(n_users, n_items) < np.where(ug[:, None] == ig[None, :], p_in, p_out)).astype(np.int8)
    holdout = np.empty(n_users, dtype=np.int64)
    for u in range(n_users):
        liked = np.flatnonzero(dense[u])
        assert len(liked) >= 2
        holdout[u] = liked[rng.randint(len(liked))]
        dense[u, holdout[u]] = 0
    return dense, holdout


def holdout_auc(scores, train, holdout):
    """mean over users of the share of unseen items ranked below the held-out one (ties count half)"""
    total = 0.0
    for u in range(train.shape[0]):
        others = np.flatnonzero(train[u] == 0)
        others = others[others != holdout[u]]
        s = scores[u, holdout[u]]
        total += ((s > scores[u, others]).sum() + 0.5 * (s == scores[u, others]).sum()) / len(others)
    return total / train.shape[0]


def top_lists(scores, topk, seen):
    """rows of `scores` -> topk column ids by descending score, ties by ascending id; seen: a 0/1 array masked out"""
    s = np.where(seen > 0, -np.inf, scores)
    return np.stack([np.lexsort((np.arange(s.shape[1]), -row))[:topk] for row in s]).astype(np.int64)
