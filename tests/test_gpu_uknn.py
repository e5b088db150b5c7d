"""The neighbour pass without an image (pk_spsp_knn_f64) bit for bit against the NumPy / SciPy restatement of its contract
(tests/uknn_reference.py) around the wave quarter (512 columns), the window (2 048) and the merge (2 x 1 024 keys), on
short and long left rows, ties across a window, stored zeros, negative values and inner indices out of range; the scoring
entry with a separate seen set (pk_spsp_topk_seen); UserKNNModel: weights, lists, scores, slices and lifecycle; and the
`gram = 'sparse'` route of ItemKNNModel and RP3BetaModel.

The restatement is computed once per input (cached below) and never written to."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import i2i_reference as i2i_ref
import knn_reference as knn_ref
import sim_reference as sim_ref
import uknn_reference as ref
from item_model_helpers import cached_fixture, limits_case, model

pytestmark = pytest.mark.gpu

N_COLS = [1, 511, 512, 513, 2047, 2048, 2049, 4097]       # the wave quarter is 512 columns, the window 2048
KINDS = {'scale': ref.SCALE, 'cosine': ref.COSINE, 'tanimoto': ref.TANIMOTO}
N_INNER = 140
LENGTHS = (0, 1, 64, 65, 130, 3, 17, 130, 2)               # entries of the left rows: around one and two wave loads of 64


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64) if x.dtype == np.float64 else x


def _same_slots(got, want):
    """count, idx, val and the pads, bit for bit."""
    for g, w, name in zip(got, want, ('count', 'idx', 'val')):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(_bits(g), _bits(w)), (name, int((_bits(g) != _bits(w)).sum()))


def _raw_csr(hip_ops, indptr, indices, values, shape, dtype=np.float64):
    """A DeviceCSR of exactly these arrays (no validation, the given value type)."""
    import torch
    from polara_amd.ops import DeviceCSR
    dev = hip_ops.device
    return DeviceCSR.from_device(hip_ops, torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(values, dtype=dtype)).to(dev), shape)


def _scipy_csr(hip_ops, S, dtype=np.float64):
    S = ref.canonical(S)
    return _raw_csr(hip_ops, S.indptr, S.indices, S.data, S.shape, dtype)


def _slots(hip_ops, *args, **kw):
    return tuple(hip_ops.to_host(x) for x in hip_ops.spsp_knn_slots(*args, **kw))


# ---- the kernel at the quarter, window and merge edges -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _crafted(n_cols):
    """(raw left rows with two inner indices out of range, B, row, col, exclude, g).  The left values are exact in fp32
    (-1, 0, 0.25, 1, 2, 3: negative and stored-zero entries), the values of B are multiples of 0.1 (their sums depend on
    the order, stored zeros among them); beyond one window every even column repeats the column 2 048 before it, so its
    weights tie with a column of the previous window."""
    rng = np.random.default_rng(100 + n_cols)
    stored = rng.random((N_INNER, n_cols)) < 0.5
    vals = rng.integers(-3, 8, (N_INNER, n_cols)) * 0.1
    col = rng.integers(0, 4, n_cols) * 0.5                             # zeros: x / 0 for the cosine without shrinkage
    for j in range(2048, n_cols, 2):
        stored[:, j], vals[:, j], col[j] = stored[:, j - 2048], vals[:, j - 2048], col[j - 2048]
    r, c = np.nonzero(stored)
    B = sps.csr_matrix((vals[r, c], (r, c)), shape=(N_INNER, n_cols))
    assert (B.data == 0).any() or n_cols == 1
    indptr, indices, values = [0], [], []
    for k, n in enumerate(LENGTHS):
        ind = list(np.sort(rng.choice(N_INNER, n, replace=False)))
        val = list(rng.choice([-1.0, 0.0, 0.25, 1.0, 2.0, 3.0], n, p=[0.1, 0.1, 0.2, 0.3, 0.2, 0.1]))
        if k in (5, 6):                                                # an inner index past the end and a negative one
            ind[1:1], val[1:1] = [N_INNER + 3, -2], [5.0, 7.0]
        indices += ind
        values += val
        indptr.append(len(indices))
    indptr, indices, values = np.array(indptr), np.array(indices, dtype=np.int64), np.array(values)
    inside = (indices >= 0) & (indices < N_INNER)
    rows = np.repeat(np.arange(len(LENGTHS)), np.diff(indptr))
    clean = sps.csr_matrix((values[inside], indices[inside], np.concatenate(([0], np.cumsum(np.bincount(rows[inside], minlength=len(LENGTHS)))))),
                           shape=(len(LENGTHS), N_INNER))
    g = ref.product(clean, B)
    row = np.array([1.0, 2.0, 0.5, 3.0, 1.5, 0.0, 2.5, 1.0, 4.0])       # a zero: every quotient of row 5 may be x / 0
    exclude = ((np.arange(len(LENGTHS)) * 37 + 11) % n_cols).astype(np.int32)
    exclude[3] = -1                                                    # nothing is excluded from row 3
    for a in (g, row, col, exclude):
        a.setflags(write=False)
    return (indptr, indices, values), B, row, col, exclude, g


@functools.lru_cache(maxsize=None)
def _crafted_rank(n_cols, kind, shrink, excluded):
    _, _, row, col, exclude, g = _crafted(n_cols)
    return ref.ranked(g, KINDS[kind], row, col, shrink, exclude if excluded else None)


@pytest.mark.parametrize('n_cols', N_COLS)
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_neighbour_pass_is_bit_equal_at_the_edges(n_cols, kind, hip_ops):
    (indptr, indices, values), B, row, col, exclude, g = _crafted(n_cols)
    Bd = _scipy_csr(hip_ops, B)
    shape = (len(LENGTHS), N_INNER)
    lefts = [_raw_csr(hip_ops, indptr, indices, values, shape, dt) for dt in (np.float32, np.float64)]
    assert [L.val_kind for L in lefts] == [0, 1]
    assert np.array_equal(hip_ops.to_host(hip_ops.spsp_rows(lefts[1], Bd)), g)          # the sums themselves: SciPy's bits
    for shrink in (0.0, 1.5):
        for excluded in (True, False):
            rank = _crafted_rank(n_cols, kind, shrink, excluded)
            for K in ((1, 2, 3, 100, 1024) if shrink == 0.0 else (3, 100)):
                for normalize in (False, True):
                    want = knn_ref.prune_ranked(rank, K, normalize)
                    for L in lefts:
                        got = _slots(hip_ops, L, Bd, KINDS[kind], row, col, shrink, K, normalize,
                                     exclude=exclude if excluded else None)
                        _same_slots(got, want)
    count = knn_ref.prune_ranked(_crafted_rank(n_cols, kind, 0.0, True), 1024, False)[0]
    assert count[0] == 0 and (count <= min(n_cols, 1024)).all()        # the empty left row; fewer candidates than K: pads
    if n_cols >= 513:
        assert count.max() > 100 and count[1] <= count[4]
    if n_cols == 4097:
        w, order = _crafted_rank(n_cols, kind, 0.0, False)
        assert max(len(o) for o in order) > 1024                       # more candidates than the largest K: the merge decides
        ties = [(r, j) for r in range(len(LENGTHS)) for j in order[r][:1024] if j >= 2048 and j % 2 == 0
                and w[r, j] == w[r, j - 2048] and (j - 2048) in order[r]]
        assert ties                                                    # equal weights on both sides of a window boundary
        r, j = ties[0]
        assert list(order[r]).index(j - 2048) < list(order[r]).index(j)                   # the lower column first


def test_negative_weights_and_the_absolute_sum(hip_ops):
    _, B, row, col, exclude, g = _crafted(2049)
    count, idx, val = knn_ref.prune_ranked(_crafted_rank(2049, 'scale', 0.0, True), 1024, True)
    assert (val < 0).any() and (g < 0).any()
    sums = np.abs(val).sum(1)
    assert np.allclose(sums[count > 0], 1.0, rtol=1e-12, atol=0)


@functools.lru_cache(maxsize=None)
def _chunked():
    """14 600 rows of 1 to 3 entries over 8 dense-ish rows of B with 4 097 columns: K = 1 024 cuts the rows into two chunks
    (pk_i2i_chunk_users = 14 563), every row has more candidates than K, and its list is merged from three windows."""
    rng = np.random.default_rng(77)
    n_rows, n_inner, n_cols = 14600, 8, 4097
    Bd = np.where(rng.random((n_inner, n_cols)) < 0.7, rng.integers(1, 9, (n_inner, n_cols)) * 0.1, 0.0)
    per = rng.integers(1, 4, n_rows)
    indptr = np.concatenate(([0], np.cumsum(per)))
    indices = np.concatenate([np.sort(rng.choice(n_inner, k, replace=False)) for k in per])
    values = rng.choice([0.5, 1.0, 2.0], len(indices))
    L = sps.csr_matrix((values, indices, indptr), shape=(n_rows, n_inner))
    row, col = rng.integers(1, 5, n_rows) * 0.5, rng.integers(1, 5, n_cols) * 0.5
    return L, sps.csr_matrix(Bd), row, col


def test_two_row_chunks(hip_ops):
    from polara_amd import _lib
    L, B, row, col = _chunked()
    n_rows, n_cols, K = L.shape[0], B.shape[1], 1024
    chunk = _lib.load().pk_i2i_chunk_users(n_rows, n_cols, K)
    assert 0 < chunk < n_rows < 2 * chunk
    got = _slots(hip_ops, _scipy_csr(hip_ops, L, np.float32), _scipy_csr(hip_ops, B), ref.COSINE, row, col, 0.5, K, True)
    # every row of the second chunk, the rows on both sides of the cut and the first rows, bit for bit
    for lo, hi in ((0, 150), (chunk - 100, n_rows)):
        want = ref.slots(ref.product(L[lo:hi], B), ref.COSINE, row[lo:hi], col, 0.5, K, True)
        _same_slots(tuple(x[lo:hi] for x in got), want)
    # every row: the count is that of the restatement's candidates, the columns ascend, the pads are pads
    for lo in range(0, n_rows, 2000):
        g = ref.product(L[lo:lo + 2000], B)
        w = knn_ref.weights(g, ref.COSINE, row[lo:lo + 2000], col, 0.5)
        cand = ((g != 0) & np.isfinite(w) & (w != 0)).sum(1)
        assert np.array_equal(got[0][lo:lo + 2000], np.minimum(cand, K))
    count, idx, val = got
    assert count.min() > 0 and (count == K).any()
    pad = np.arange(K)[None, :] >= count[:, None]
    assert (idx[pad] == -1).all() and not val[pad].any() and (val[~pad] > 0).all()
    assert (np.diff(idx.astype(np.int64), axis=1)[~pad[:, 1:]] > 0).all()


def test_two_calls_give_the_same_bits(hip_ops):
    (indptr, indices, values), B, row, col, exclude, _ = _crafted(4097)
    L, Bd = _raw_csr(hip_ops, indptr, indices, values, (len(LENGTHS), N_INNER)), _scipy_csr(hip_ops, B)
    a = _slots(hip_ops, L, Bd, ref.TANIMOTO, row, col, 1.0, 100, True, exclude=exclude)
    b = _slots(hip_ops, L, Bd, ref.TANIMOTO, row, col, 1.0, 100, True, exclude=exclude)
    _same_slots(a, b)
    assert a[0].max() == 100


def test_ops_checks(hip_ops):
    from polara_amd._lib import PolaraHipError
    _, B, row, col, exclude, _ = _crafted(513)
    L = _scipy_csr(hip_ops, sps.random(9, N_INNER, 0.2, random_state=1))
    Bd = _scipy_csr(hip_ops, B)
    for K in (0, 1025):
        with pytest.raises(ValueError, match='neighbours'):
            hip_ops.spsp_knn_slots(L, Bd, ref.COSINE, row, col, 0.0, K, False)
    with pytest.raises(ValueError, match='`col`'):
        hip_ops.spsp_knn_slots(L, Bd, ref.COSINE, row, col[:-1], 0.0, 3, False)
    with pytest.raises(ValueError, match='`row`'):
        hip_ops.spsp_knn_slots(L, Bd, ref.COSINE, row[:-1], col, 0.0, 3, False)
    with pytest.raises(ValueError, match='exclude'):
        hip_ops.spsp_knn_slots(L, Bd, ref.COSINE, row, col, 0.0, 3, False, exclude=exclude[:-1])
    with pytest.raises(ValueError, match='columns'):                   # L B does not fit
        hip_ops.spsp_knn_slots(Bd, Bd, ref.COSINE, np.ones(N_INNER), col, 0.0, 3, False)
    with pytest.raises(ValueError, match='device CSR'):                # a SciPy matrix: no device addresses
        hip_ops.spsp_knn_slots(B, Bd, ref.COSINE, row, col, 0.0, 3, False)
    with pytest.raises(PolaraHipError, match='kind'):
        hip_ops.spsp_knn_slots(L, Bd, 7, row, col, 0.0, 3, False)
    with pytest.raises(PolaraHipError, match='shrink'):
        hip_ops.spsp_knn_slots(L, Bd, ref.COSINE, row, col, -1.0, 3, False)
    W = hip_ops.spsp_knn(L, Bd, ref.SCALE, np.zeros(9), col, 0.0, 3, False)               # every weight 0: the empty CSR
    assert W.shape == (9, 513) and W.nnz == 0 and not hip_ops.to_host(W.indptr).any() and W.indices.numel() == 0
    seen = _scipy_csr(hip_ops, sps.random(9, 513, 0.1, random_state=2))
    with pytest.raises(ValueError, match='seen'):
        hip_ops.spsp_topk_seen(L, Bd, L, 5, True, False)               # [9 x 140]: not over the columns of the scores
    with pytest.raises(ValueError, match='device CSR'):
        hip_ops.spsp_topk_seen(L, Bd, B, 5, True, False)
    with pytest.raises(PolaraHipError, match='topk'):
        hip_ops.spsp_topk_seen(L, Bd, seen, 1025, True, False)


# ---- scoring with a separate seen set ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _square_case():
    """L [50 x 2100] against B [2100 x 2100]: two windows, the seen set of pk_spsp_topk is L's own row."""
    rng = np.random.default_rng(41)
    n = 2100
    L = sps.random(50, n, 0.01, random_state=rng, data_rvs=lambda k: rng.integers(0, 6, k).astype(np.float64)).tocsr()
    B = sps.random(n, n, 0.004, random_state=rng, data_rvs=lambda k: rng.integers(-2, 9, k) * 0.1).tocsr()
    return ref.canonical(L), ref.canonical(B)


def test_topk_seen_with_the_left_rows_is_spsp_topk(hip_ops):
    L, B = _square_case()
    Ld, Bd = _scipy_csr(hip_ops, L, np.float32), _scipy_csr(hip_ops, B)
    assert (L.data == 0).any()                                         # zero-valued entries are seen too
    for sparse in (False, True):
        for filter_seen in (False, True):
            for topk in (1, 10, 100, 1024):
                a, sa = hip_ops.spsp_topk(Ld, Bd, topk, filter_seen, sparse, want_scores=True)
                b, sb = hip_ops.spsp_topk_seen(Ld, Bd, Ld, topk, filter_seen, sparse, want_scores=True)
                assert np.array_equal(hip_ops.to_host(a), hip_ops.to_host(b)), (sparse, filter_seen, topk)
                assert np.array_equal(_bits(hip_ops.to_host(sa)), _bits(hip_ops.to_host(sb)))
    assert hip_ops.spsp_topk_seen(Ld, Bd, Ld, 10, True, True)[1] is None


@functools.lru_cache(maxsize=None)
def _foreign_case():
    """L [40 x 130] against B [130 x 2100] with a seen set [40 x 2100] that has nothing to do with L (one row empty, one
    row seeing every column of the second window)."""
    rng = np.random.default_rng(43)
    L = sps.random(40, 130, 0.1, random_state=rng, data_rvs=lambda k: rng.integers(1, 6, k).astype(np.float64)).tocsr()
    B = sps.random(130, 2100, 0.02, random_state=rng, data_rvs=lambda k: rng.integers(-2, 9, k) * 0.1).tocsr()
    seen = rng.random((40, 2100)) < 0.2
    seen[3] = False
    seen[4, 2048:] = True
    return ref.canonical(L), ref.canonical(B), seen, sim_ref.product(L, B)


def test_topk_seen_with_a_foreign_seen_set(hip_ops):
    L, B, seen, scores = _foreign_case()
    Ld, Bd, Sd = _scipy_csr(hip_ops, L), _scipy_csr(hip_ops, B), _scipy_csr(hip_ops, sps.csr_matrix(seen.astype(np.float64)))
    for sparse in (False, True):
        for filter_seen in (False, True):
            for topk in (1, 10, 100, 1024):
                want = i2i_ref.select(scores, seen, topk, filter_seen, sparse)
                recs, s = (hip_ops.to_host(x) for x in hip_ops.spsp_topk_seen(Ld, Bd, Sd, topk, filter_seen, sparse, want_scores=True))
                assert recs.dtype == np.int64 and np.array_equal(recs, want), (sparse, filter_seen, topk)
                s_ref = np.where(want >= 0, np.take_along_axis(scores, np.maximum(want, 0), 1), 0.0)
                assert np.array_equal(_bits(s), _bits(s_ref)), (sparse, filter_seen, topk)
    unseen = i2i_ref.select(scores, seen, 1024, True, True)
    assert not seen[np.arange(40)[:, None], np.maximum(unseen, 0)][unseen >= 0].any() and (unseen[4][unseen[4] >= 0] < 2048).all()


# ---- UserKNNModel ------------------------------------------------------------------------------------------------------
_fixture = cached_fixture(ref)


@functools.lru_cache(maxsize=None)
def _user_gram(name, implicit):
    A = ref.canonical(_fixture(name, implicit)[3])
    return ref.product(A, ref.transposed(A))


def _csr_arrays(hip_ops, W):
    return tuple(hip_ops.to_host(x).copy() for x in (W.indptr, W.indices, W.values))


def _same_csr(arrays, want):
    ptr, ind, dat = arrays
    assert ptr.dtype == np.int64 and ind.dtype == np.int32 and dat.dtype == np.float64
    assert np.array_equal(ptr, want.indptr) and np.array_equal(ind, want.indices)
    assert np.array_equal(_bits(dat), _bits(want.data))


UKNN_SETTINGS = [dict(similarity='cosine', neighbours=10), dict(similarity='cosine', neighbours=25, shrink=5.0, normalize=True),
                 dict(similarity='cosine', neighbours=10, asymmetric_alpha=0.3), dict(similarity='jaccard', neighbours=10),
                 dict(similarity='jaccard', neighbours=40, shrink=2.0, normalize=True)]


def _uknn_reference(A, s, g=None):
    return ref.user_knn_weights(A, s['similarity'], s['neighbours'], s.get('shrink', 0.0), s.get('asymmetric_alpha', 0.5),
                                s.get('normalize', False), g=g)


@pytest.mark.parametrize('name,implicit', [('small', False), ('small', True), ('large', False), ('large', True)])
def test_user_weights_are_the_restatement(name, implicit, hip_ops):
    """`large`: 3 000 users, two windows of neighbours per row."""
    idx, val, shape, A = _fixture(name, implicit)
    n = shape[0]
    for s in (UKNN_SETTINGS if name == 'small' else UKNN_SETTINGS[1::2]):
        m = model('UserKNNModel', hip_ops, idx, val, shape, implicit=implicit, **s)
        m.build()
        arrays = _csr_arrays(hip_ops, m.user_weights)
        _same_csr(arrays, _uknn_reference(A, s, _user_gram(name, implicit)))
        ptr, ind, dat = arrays
        rows = np.repeat(np.arange(n), np.diff(ptr))
        assert m.user_weights.shape == (n, n) and (rows != ind).all() and (dat > 0).all() and np.diff(ptr).max() <= s['neighbours']
        st = m.build_stats
        assert {'upload_s', 'neighbours_s', 'nnz', 'neighbours', 'training_nnz', 'n_users'} <= set(st)
        assert (st['nnz'], st['neighbours'], st['n_users'], st['training_nnz']) == (len(ind), s['neighbours'], n, A.nnz)
        assert st['neighbours_s'] > 0 and m.user_weights.nnz == len(ind) > 0


def _known_users(n_users, n_items):
    """A holdout that names every 25th user: the test rows are the training rows of those users."""
    users = np.arange(3, n_users, 25)
    return users, (users, (users * 7) % n_items, np.ones(len(users)))


@pytest.mark.parametrize('settings', [dict(neighbours=10), dict(similarity='jaccard', neighbours=30, normalize=True, shrink=1.0)])
@pytest.mark.parametrize('implicit', [False, True])
@pytest.mark.parametrize('warm', [False, True])
def test_model_lists_scores_and_slices(settings, implicit, warm, hip_ops):
    """Known users (the holdout names training users: their rows of N) and warm start (the neighbours of the test rows by
    the same kernel, nobody excluded): lists and their scores are SciPy's N_test.dot(X) followed by the layer's order, in
    both branches of `dense_output`, with and without `filter_seen`; the seen set is the test row's own pattern."""
    idx, val, shape, A = _fixture('medium', implicit)
    A = ref.canonical(A)
    s = dict(similarity='cosine', shrink=0.0, normalize=False)
    s.update(settings)
    args = (s['similarity'], s['neighbours'], s['shrink'], 0.5, s['normalize'])
    if warm:
        test, holdout, tshape = ref.test_rows('medium')
        T, seen = i2i_ref.test_matrix(test, tshape, implicit)
        N_test = ref.user_neighbours(T, A, *args)
        assert N_test[2].nnz == s['neighbours'] and not N_test[1].nnz and not N_test[-1].nnz     # zero-feedback and empty rows
    else:
        users, holdout = _known_users(*shape)
        test, tshape = None, (len(users), shape[1])
        N_test = ref.user_knn_weights(A, *args, g=_user_gram('medium', implicit))[users]
        seen = sim_ref.seen_mask(A[users])
        assert not (N_test.indices == np.repeat(users, np.diff(N_test.indptr))).any()               # nobody is its own neighbour
    scores = ref.scores(N_test, A)
    m = model('UserKNNModel', hip_ops, idx, val, shape, test, holdout, implicit=implicit, **settings)
    m.build()
    for dense_output in (True, False):
        m.dense_output = dense_output
        for filter_seen in (True, False):
            cls_ = i2i_ref.classes(scores, seen, filter_seen, not dense_output)
            for topk in (1, 10, 100):
                m.filter_seen, m.topk = filter_seen, topk
                recs = m.get_recommendations()
                want = i2i_ref.select(scores, seen, topk, filter_seen, not dense_output)
                assert recs.shape == want.shape and recs.dtype == np.int64
                assert i2i_ref.tie_aware_mismatches(recs, want, scores, cls_, tol=0.0) == [], (dense_output, filter_seen, topk)
                assert np.array_equal(recs, want), (dense_output, filter_seen, topk)
                lists, list_scores = m.recommend_with_scores()
                assert np.array_equal(lists, recs)
                s_ref = np.where(lists >= 0, np.take_along_axis(scores, np.maximum(lists, 0), 1), 0.0)
                assert np.array_equal(_bits(list_scores), _bits(s_ref)), (dense_output, filter_seen, topk)
    assert len(m.training_time) == 1                                            # none of this rebuilt the model
    test_data, test_shape, test_users = m._get_test_data()
    assert tuple(test_shape) == tuple(tshape)
    block, triplet = m.slice_recommendations(test_data, test_shape, 3, 17)      # the sparse branch: a SciPy CSR
    assert sps.issparse(block) and block.shape == (14, shape[1])
    assert np.array_equal(block.toarray(), scores[3:17]) and (block.data != 0).all()
    m.dense_output = True
    block, triplet = m.slice_recommendations(test_data, test_shape, 3, 17, test_users)
    assert isinstance(block, np.ndarray) and np.array_equal(_bits(block), _bits(scores[3:17]))
    assert m._slice_users is None


def test_user_knn_lifecycle(hip_ops):
    idx, val, shape, _ = _fixture('medium', False)
    test, holdout, tshape = ref.test_rows('medium')
    m = model('UserKNNModel', hip_ops, idx, val, shape, test, holdout, neighbours=20)
    m.topk = 10
    recs = m.recommendations
    first = _csr_arrays(hip_ops, m.user_weights)
    assert recs.shape == (tshape[0], 10) and len(m.training_time) == 1
    m.similarity, m.neighbours, m.shrink, m.asymmetric_alpha, m.normalize, m.implicit = 'cosine', 20, 0, 0.5, False, False
    assert m.recommendations is recs and m._is_ready and len(m.training_time) == 1          # unchanged: nothing happens
    N = m.user_weights
    m.dense_output = False                                      # the other branch: new lists, the same model
    assert m.recommendations.shape == recs.shape and m.user_weights is N and len(m.training_time) == 1
    m.dense_output = True
    builds = 1
    for name, value in (('similarity', 'jaccard'), ('neighbours', 7), ('shrink', 3.0), ('asymmetric_alpha', 0.2),
                        ('normalize', True), ('implicit', True)):
        setattr(m, name, value)                                 # a change: the weights are dropped at once, then rebuilt
        assert m.user_weights is None and m._operand() is None and not m._is_ready, name
        other = m.recommendations
        builds += 1
        assert len(m.training_time) == builds and m.user_weights is not None and other.shape == recs.shape
    m.similarity, m.neighbours, m.shrink, m.asymmetric_alpha, m.normalize, m.implicit = 'cosine', 20, 0, 0.5, False, False
    assert np.array_equal(m.recommendations, recs)
    again = _csr_arrays(hip_ops, m.user_weights)                # the first settings again: the first weights, bit for bit
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, again))
    assert m.evaluate(topk=10) is not None
    m.data.set_training_data((idx[:, 0], idx[:, 1], val * 2))    # a data change: a new model
    assert m.user_weights is None and not m._is_ready
    bad = val.copy()
    bad[[3, 10, 50]] = -1.0
    m = model('UserKNNModel', hip_ops, idx, bad, shape, test, holdout)
    with pytest.raises(ValueError, match='3 of %d' % len(bad)):
        m.build()


def test_stated_limits(hip_ops):
    """More items than the 1024 of a list, and every user a test user (the rows of N as they are, no gather)."""
    pairs, val, (n_users, n_items), hold = limits_case()
    m = model('UserKNNModel', hip_ops, pairs, val, (n_users, n_items), holdout=hold, neighbours=1024)
    m.topk = 1024
    assert m.recommendations.shape == (n_users, 1024) and m.user_weights.shape == (n_users, n_users)
    m.topk = 1025
    with pytest.raises(ValueError, match='1024'):
        m.get_recommendations()
    with pytest.raises(ValueError, match='1024'):
        m.recommend_with_scores()


# ---- gram = 'sparse' ---------------------------------------------------------------------------------------------------
KNN_SETTINGS = [dict(similarity='cosine', neighbours=10), dict(similarity='cosine', neighbours=25, shrink=5.0, normalize=True,
                                                              asymmetric_alpha=0.3),
                dict(similarity='jaccard', neighbours=40, shrink=2.0, normalize=True)]
RP3_SETTINGS = [dict(neighbours=10), dict(neighbours=25, alpha=0.7, beta=0.4, normalize=True)]


def _no_image(hip_ops, monkeypatch):
    """The sparse route allocates no image and does not consult the memory guard."""
    from polara_amd import i2i

    def refuse(*a, **k):
        raise AssertionError('the sparse route must not touch the Gram image')
    monkeypatch.setattr(hip_ops, 'knn_gram', refuse)
    monkeypatch.setattr(i2i, 'check_build_memory', refuse)


@pytest.mark.parametrize('name,implicit', [('small', False), ('small', True), ('medium', False)])
def test_sparse_route_weights_are_the_restatement(name, implicit, hip_ops, monkeypatch):
    idx, val, shape, A = _fixture(name, implicit)
    n = shape[1]
    _no_image(hip_ops, monkeypatch)
    for s in KNN_SETTINGS:
        m = model('ItemKNNModel', hip_ops, idx, val, shape, implicit=implicit, gram='sparse', **s)
        m.build()
        want = ref.item_knn_sparse_weights(A, s['similarity'], s['neighbours'], s.get('shrink', 0.0), s.get('asymmetric_alpha', 0.5),
                                           s.get('normalize', False))
        _same_csr(_csr_arrays(hip_ops, m.item_weights), want)
        st = m.build_stats
        assert (st['gram'], st['image_bytes'], st['nnz'], st['n_items']) == ('sparse', 0, want.nnz, n) and st['transpose_s'] > 0
    for s in RP3_SETTINGS:
        m = model('RP3BetaModel', hip_ops, idx, val, shape, implicit=implicit, gram='sparse', **s)
        m.build()
        want = ref.rp3_sparse_weights(A, s.get('alpha', 1.0), s.get('beta', 0.6), s['neighbours'], s.get('normalize', False))
        arrays = _csr_arrays(hip_ops, m.item_weights)
        _same_csr(arrays, want)
        rows = np.repeat(np.arange(n), np.diff(arrays[0]))
        assert (rows != arrays[1]).all() and m.build_stats['transpose_s'] == 0.0 and m.build_stats['gram'] == 'sparse'


def test_sparse_route_is_the_image_route_on_integer_feedback(hip_ops):
    """Integer feedback: both Gram matrices are exact, so the two routes give the same ItemKNN weights bit for bit, and the
    same lists."""
    idx, val, shape, A = _fixture('medium', False)
    test, holdout, tshape = ref.test_rows('medium')
    assert np.array_equal(val, np.round(val))
    for s in KNN_SETTINGS:
        built = []
        for gram in ('image', 'sparse'):
            m = model('ItemKNNModel', hip_ops, idx, val, shape, test, holdout, gram=gram, **s)
            m.build()
            assert m.build_stats['gram'] == gram and (m.build_stats['image_bytes'] > 0) == (gram == 'image')
            built.append((_csr_arrays(hip_ops, m.item_weights), m.get_recommendations()))
        (a, ra), (b, rb) = built
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b)) and len(a[1]) > 0
        assert np.array_equal(ra, rb)
    m.gram = 'image'                                             # a change of the route renews the model
    assert m.item_weights is None and not m._is_ready
