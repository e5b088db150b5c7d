"""NumPy / SciPy restatement of the item-to-item and most-popular baselines under the total order of the device path
(polara_amd.models.CooccurrenceModel / PopularityModel): key of an item = (class, score), class 2 = candidate,
1 = seen item of the dense branch under filter_seen, 0 = not a candidate (pad, -1); ties go to the lower item index.
tests/test_i2i_host.py pins it against the reference's own lists (tests/golden/i2i_*.npz); the GPU tests compare the
device lists with it exactly."""
import numpy as np
import scipy.sparse as sps


def training_matrix(idx, val, shape, implicit=False):
    A = sps.csr_matrix((np.asarray(val, dtype=np.float64), (idx[:, 0], idx[:, 1])), shape=tuple(shape))
    A.sum_duplicates()
    if implicit:
        A.data = np.sign(A.data)
    return A


def i2i_matrix(A):
    """Dense C = A^T A with the diagonal set to 0 (models.py:710-713)."""
    C = (A.T @ A).toarray()
    np.fill_diagonal(C, 0)
    return C


def test_matrix(test_data, shape, implicit=False):
    """(CSR of the test entries with nonzero feedback, boolean seen mask of every entry) of test rows x items."""
    u, i, f = (np.asarray(x) for x in test_data)
    f = np.asarray(f, dtype=np.float64)
    if implicit:
        f = np.sign(f)
    keep = f != 0
    T = sps.csr_matrix((f[keep], (u[keep], i[keep])), shape=tuple(shape[:2]))
    seen = np.zeros(tuple(shape[:2]), dtype=bool)
    seen[u, i] = True
    return T, seen


def i2i_scores(C, T):
    return np.asarray(T @ C)


def popularity_scores(idx, val, n_items, by_feedback_value=False):
    w = np.asarray(val, dtype=np.float64) if by_feedback_value else None
    return np.bincount(np.asarray(idx[:, 1], dtype=np.int64), weights=w, minlength=n_items).astype(np.float64)


def classes(scores, seen, filter_seen, sparse):
    sn = seen & bool(filter_seen)
    if sparse:
        return np.where((scores != 0) & ~sn, 2, 0)
    return np.where(sn, 1, 2)


def select(scores, seen, topk, filter_seen, sparse):
    """[n_rows x topk] lists under (class desc, score desc, item asc), -1 where a row runs out of candidates."""
    cls = classes(scores, seen, filter_seen, sparse)
    n_rows, n_items = scores.shape
    out = np.full((n_rows, topk), -1, dtype=np.int64)
    items = np.arange(n_items)
    for r in range(n_rows):
        order = np.lexsort((items, -scores[r], -cls[r]))[:topk]
        order = order[cls[r, order] > 0]
        out[r, :len(order)] = order
    return out


def tie_aware_mismatches(recs, ref, scores, cls, tol=0.0):
    """Rows where `recs` and `ref` differ beyond ties: per row the pads sit at the same positions, the key (class, score)
    at every position is the same, and the items whose key is strictly better than the key at position topk - 1 are the
    same set.  `tol` > 0 (feedback that is not exactly representable: sums in another order differ in the last bits):
    scores within tol * max(1, |score|) of each other count as tied.  Returns the list of offending row numbers."""
    bad = []
    for r in range(recs.shape[0]):
        a, b = recs[r], ref[r]
        if not np.array_equal(a < 0, b < 0):
            bad.append(r)
            continue
        live = a >= 0
        if not live.any():
            continue
        ca, cb = cls[r, a[live]], cls[r, b[live]]
        sa, sb = scores[r, a[live]], scores[r, b[live]]
        if not (np.array_equal(ca, cb) and np.all(np.abs(sa - sb) <= tol * np.maximum(1, np.abs(sb)))):
            bad.append(r)
            continue
        lc, ls = cb[-1], sb[-1]
        eps = tol * max(1.0, abs(ls))

        def strict(items, c, s):
            return {int(x) for x, ci, si in zip(items, c, s) if ci > lc or (ci == lc and si > ls + eps)}
        if strict(a[live], ca, sa) != strict(b[live], cb, sb):
            bad.append(r)
    return bad


def fixture_lists(g):
    """(scores, classes, lists under the total order) of a tests/golden/i2i_*.npz fixture, from its inputs."""
    shape = tuple(int(x) for x in g['test_shape'])
    topk, fs = int(g['topk']), bool(g['filter_seen'])
    T, seen = test_matrix((g['test_user'], g['test_item'], g['test_fdbk']), shape, bool(g['implicit']))
    if str(g['model']) == 'MP':
        s = popularity_scores(g['train_idx'], g['train_val'], shape[1], bool(g['by_feedback_value']))
        scores = np.repeat(s[None, :], shape[0], axis=0)
        sparse = False
    else:
        A = training_matrix(g['train_idx'], g['train_val'], tuple(g['train_shape']), bool(g['implicit']))
        scores = i2i_scores(i2i_matrix(A), T)
        sparse = not bool(g['dense_output'])
    return scores, classes(scores, seen, fs, sparse), select(scores, seen, topk, fs, sparse)
