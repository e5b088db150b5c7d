"""ItemKNN and RP3beta on the device: the pruning pass (pk_knn_prune_f64) bit for bit against the NumPy restatement of its
contract (tests/knn_reference.py) around the window (2 048 columns) and the merge (2 x 1 024 keys), on degenerate and tied
items and on a crafted image with negative entries; the Gram image of the RP3beta transform within its derived bound; and
the models: the canonical weights, lists, scores, slices, lifecycle and limits.

The restatement is computed once per input (cached below) and never written to."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import i2i_reference as i2i_ref
import knn_reference as ref
from item_model_helpers import cached_fixture, device_csr as _device_csr, limits_case, model

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 17, 63, 64, 65, 257, 1025, 2050]        # all but 64 no multiple of 8 (ldg != n); past one window and past 2 x 1024 keys
KINDS = {'scale': ref.SCALE, 'cosine': ref.COSINE, 'tanimoto': ref.TANIMOTO}


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64) if x.dtype == np.float64 else x


def _same_slots(got, want):
    """count, idx, val and the pads, bit for bit."""
    for g, w, name in zip(got, want, ('count', 'idx', 'val')):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(_bits(g), _bits(w)), (name, int((_bits(g) != _bits(w)).sum()))


def _device_slots(hip_ops, G, n, kind, row, col, shrink, K, normalize):
    return tuple(hip_ops.to_host(x) for x in hip_ops.knn_prune_slots(G, n, kind, row, col, shrink, K, normalize))


# ---- the kernel at the window and merge edges ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sized_case(n):
    """Integer feedback 1..5 over n items; beyond 16 items one item loses its entries (a zero norm) and one item becomes
    the copy of another (equal weights everywhere: ties that go to the lower column)."""
    idx, val, shape = ref.sized_training(n)
    empty = twin = None
    if n > 16:
        empty, src, twin = 5, 3, 11
        keep = (idx[:, 1] != empty) & (idx[:, 1] != twin)
        copy = idx[idx[:, 1] == src].copy()
        copy[:, 1] = twin
        idx, val = np.concatenate([idx[keep], copy]), np.concatenate([val[keep], val[idx[:, 1] == src]])
        order = np.lexsort((idx[:, 1], idx[:, 0]))
        idx, val = idx[order], val[order]
    return idx, val, shape, empty, twin


def _vectors(kind, q):
    """(row, col) of a kind from the diagonal q: an asymmetric cosine, the plain Tanimoto, and a walk-like scaling."""
    if kind == 'cosine':
        return ref.power(q, 0.7), ref.power(q, 0.3)
    if kind == 'tanimoto':
        return q, q
    return ref.inverse_power(q, 1.0), ref.inverse_power(q, 0.4)


@functools.lru_cache(maxsize=None)
def _sized_rank(n, kind, shrink):
    idx, val, shape, _, _ = _sized_case(n)
    G = ref.gram(ref.training_matrix(idx, val, shape))
    row, col = _vectors(kind, np.ascontiguousarray(np.diagonal(G)))
    return ref.ranked(G, KINDS[kind], row, col, shrink)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_prune_is_bit_equal_at_the_edges(n, kind, hip_ops):
    from polara_amd import i2i
    idx, val, shape, empty, twin = _sized_case(n)
    G = hip_ops.knn_gram(_device_csr(hip_ops, idx, val, shape))
    Gh = hip_ops.to_host(G)
    assert G.shape == (n, i2i.leading_dim(n)) and (G.stride(0) != n) == (n % 8 != 0) and not Gh[:, n:].any()
    Gh = np.ascontiguousarray(Gh[:, :n])
    assert np.array_equal(Gh, ref.gram(ref.training_matrix(idx, val, shape)))          # integer feedback: exact
    row, col = _vectors(kind, np.ascontiguousarray(np.diagonal(Gh)))
    for shrink in (0.0, 5.0):
        rank = _sized_rank(n, kind, shrink)
        for K in sorted({1, 10, max(1, min(n - 1, 1024)), 1024}):
            for normalize in (False, True):
                want = ref.prune_ranked(rank, K, normalize)
                got = _device_slots(hip_ops, G, n, KINDS[kind], row, col, shrink, K, normalize)
                _same_slots(got, want)
                count, ind, dat = got
                if empty is not None:
                    assert count[empty] == 0 and (ind[empty] == -1).all() and not dat[empty].any()      # 0 / 0 or g = 0
                    assert not (ind == empty).any()
                if K == 1024:
                    assert count.max() < K or n > K                     # rows with fewer than K candidates: pads
                    assert (ind[np.arange(K)[None, :] >= count[:, None]] == -1).all()
    if twin is not None:
        w, order = _sized_rank(n, kind, 0.0)
        rows = [i for i in range(n) if i not in (3, twin) and 3 in order[i]]
        assert rows and all(w[i, 3] == w[i, twin] for i in rows)        # the twins tie in every row that sees them
        assert all(list(order[i]).index(3) < list(order[i]).index(twin) for i in rows)      # the lower column first


# ---- a crafted image: not symmetric, negative entries, infinities, both load paths --------------------------------------
@functools.lru_cache(maxsize=None)
def _crafted(n=300):
    rng = np.random.default_rng(19)
    G = np.where(rng.random((n, n)) < 0.6, np.round(rng.standard_normal((n, n)) * 8) / 4, 0.0)
    G[7] = -np.abs(G[7])                                               # a row of negative entries only
    G[8, :] = 0.0                                                      # a row without candidates
    G[9, 20:] = 0.0                                                    # a row with fewer candidates than most K
    row, col = rng.integers(1, 5, n).astype(np.float64), rng.integers(1, 5, n).astype(np.float64)
    row[3] = 0.0                                                       # cosine, shrink 0: every quotient of row 3 is x / 0
    col[4] = 0.0
    G.setflags(write=False)
    return G, row, col


@functools.lru_cache(maxsize=None)
def _crafted_rank(kind, shrink):
    G, row, col = _crafted()
    return ref.ranked(G, KINDS[kind], row, col, shrink)


@pytest.mark.parametrize('ld', [300, 301, 304])
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_crafted_image_with_negative_entries(ld, kind, hip_ops):
    """ld 304: whole 16-byte loads; 300 and 301: the row stride is no multiple of 8 (301: rows are not even 16-byte
    aligned), one double at a time.  The same bits."""
    import torch
    G, row, col = _crafted()
    n = G.shape[0]
    image = np.full((n, ld), 7.0)
    image[:, :n] = G
    Gd = torch.from_numpy(image).to(hip_ops.device)
    for shrink in (0.0, 5.0):
        rank = _crafted_rank(kind, shrink)
        for K in (1, 10, 299, 1024):
            for normalize in (False, True):
                want = ref.prune_ranked(rank, K, normalize)
                got = _device_slots(hip_ops, Gd, n, KINDS[kind], row, col, shrink, K, normalize)
                _same_slots(got, want)
    count, ind, dat = ref.prune_ranked(_crafted_rank(kind, 0.0), 299, False)
    assert count[8] == 0 and count[9] <= 20 and (dat < 0).any()
    pos, neg = (dat > 0).sum(1), (dat < 0).sum(1)
    assert ((pos > 0) & (neg > 0)).any()                               # negative weights kept below positive ones
    if kind == 'cosine':
        assert count[3] == 0 and not (ind == 4).any()                  # x / 0: infinite, no candidate
    if kind == 'scale':
        assert (dat[7, :count[7]] < 0).all() and count[7] > 0
        s = ref.prune_ranked(_crafted_rank(kind, 0.0), 299, True)[2][7]
        assert np.isclose(-s.sum(), 1.0, rtol=1e-13)                    # the ABSOLUTE sum normalises a negative row


def test_two_calls_give_the_same_bits(hip_ops):
    idx, val, shape, _, _ = _sized_case(1025)
    G = hip_ops.knn_gram(_device_csr(hip_ops, idx, val, shape))
    q = hip_ops.to_host(G.diagonal()).copy()
    row, col = _vectors('cosine', q)
    a = _device_slots(hip_ops, G, 1025, ref.COSINE, row, col, 1.0, 100, True)
    b = _device_slots(hip_ops, G, 1025, ref.COSINE, row, col, 1.0, 100, True)
    _same_slots(a, b)
    assert a[0].max() == 100


def test_ops_checks(hip_ops):
    import torch
    from polara_amd._lib import PolaraHipError
    G = torch.zeros(5, 8, dtype=torch.float64, device=hip_ops.device)
    v = np.ones(5)
    for K in (0, 1025):
        with pytest.raises(ValueError, match='neighbours'):
            hip_ops.knn_prune_slots(G, 5, ref.COSINE, v, v, 0.0, K, False)
    with pytest.raises(ValueError, match='col'):
        hip_ops.knn_prune_slots(G, 5, ref.COSINE, v, np.ones(4), 0.0, 3, False)
    with pytest.raises(ValueError, match='image'):
        hip_ops.knn_prune_slots(G, 9, ref.COSINE, np.ones(9), np.ones(9), 0.0, 3, False)
    with pytest.raises(ValueError, match='image'):                     # a host tensor: its address is no device pointer
        hip_ops.knn_prune_slots(G.cpu(), 5, ref.COSINE, v, v, 0.0, 3, False)
    with pytest.raises(PolaraHipError, match='kind'):
        hip_ops.knn_prune_slots(G, 5, 7, v, v, 0.0, 3, False)
    with pytest.raises(PolaraHipError, match='shrink'):
        hip_ops.knn_prune_slots(G, 5, ref.COSINE, v, v, -1.0, 3, False)
    W = hip_ops.knn_prune(G, 5, ref.COSINE, v, v, 0.0, 3, False)       # an all-zero image: the empty CSR
    assert W.shape == (5, 5) and W.nnz == 0 and not hip_ops.to_host(W.indptr).any() and W.indices.numel() == 0


# ---- the Gram image of the RP3beta transform ---------------------------------------------------------------------------
_fixture = cached_fixture(ref)


@functools.lru_cache(maxsize=None)
def _synthetic():
    """The 300-item case: ref.sized_training(300) as a fixture tuple."""
    idx, val, shape = ref.sized_training(300)
    return idx, val, shape, ref.training_matrix(idx, val, shape)


@functools.lru_cache(maxsize=None)
def _fractional():
    """`small` with its feedback times 0.3: values that are not exact, so the row and column sums depend on their order."""
    idx, val, shape = ref.training('small')
    val = val * 0.3
    return idx, val, shape, ref.training_matrix(idx, val, shape)


def _case(name, implicit=False):
    if name == 'fractional':
        assert not implicit
        return _fractional()
    if name == 'synthetic':
        idx, val, shape, A = _synthetic()
        return (idx, val, shape, ref.training_matrix(idx, val, shape, implicit)) if implicit else (idx, val, shape, A)
    return _fixture(name, implicit)


@pytest.mark.parametrize('name', ['small', 'synthetic', 'fractional'])
def test_gram_of_the_rp3_transform(name, hip_ops):
    """alpha = 0.7: X' is bit-equal to the restatement's, and every entry of the device image is within 2 gamma_m relative
    of NumPy's Gram matrix of the same X' — both sides sum at most m non-negative rounded products (m: the largest item
    count), each within gamma_m of the exact sum, so the bound is derived, not measured.  `fractional`: feedback whose sums are not exact in any order —
    the device CSR and the restatement's SciPy CSR are both canonical (row-major, sorted columns) and both sum with
    np.bincount in that storage order, so d_u, d_i and with them X', r and c are still the same bits."""
    idx, val, shape, A = _case(name)
    m = model('RP3BetaModel', hip_ops, idx, val, shape, alpha=0.7)
    X, r, c = m._transformed(m._training_device_csr())
    Xr, rr, cr = ref.rp3_parts(A, 0.7, m.beta)
    assert X.values.dtype.itemsize == 8 and np.array_equal(hip_ops.to_host(X.indptr), Xr.indptr)
    assert np.array_equal(hip_ops.to_host(X.indices), Xr.indices)
    assert np.array_equal(_bits(hip_ops.to_host(X.values)), _bits(Xr.data))
    assert np.array_equal(_bits(r), _bits(rr)) and np.array_equal(_bits(c), _bits(cr))
    n = shape[1]
    Gh = hip_ops.to_host(hip_ops.knn_gram(X))[:, :n]
    want = ref.gram(Xr)
    items = int(np.diff(A.tocsc().indptr).max())
    assert np.array_equal(Gh != 0, want != 0)
    nz = want != 0
    gap = float((np.abs(Gh[nz] - want[nz]) / want[nz]).max())
    print('largest relative gap %.3g u, bound %.3g u (m = %d)' % (gap / ref.U, 2 * ref.gamma(items) / ref.U, items))
    assert gap <= 2 * ref.gamma(items)


# ---- models --------------------------------------------------------------------------------------------------------------
def _csr_arrays(hip_ops, W):
    return tuple(hip_ops.to_host(x).copy() for x in (W.indptr, W.indices, W.values))


def _same_csr(arrays, want):
    ptr, ind, dat = arrays
    assert ptr.dtype == np.int64 and ind.dtype == np.int32 and dat.dtype == np.float64
    assert np.array_equal(ptr, want.indptr) and np.array_equal(ind, want.indices)
    assert np.array_equal(_bits(dat), _bits(want.data))


def _is_canonical(arrays, n, per_row=None, per_column=None):
    ptr, ind, dat = arrays
    rows = np.repeat(np.arange(n), np.diff(ptr))
    assert (rows != ind).all() and (dat != 0).all() and np.isfinite(dat).all()          # no diagonal, no stored zero
    assert all((np.diff(ind[ptr[r]:ptr[r + 1]]) > 0).all() for r in range(n))            # sorted, no duplicates
    if per_row is not None:
        assert np.diff(ptr).max() <= per_row
    if per_column is not None:
        assert np.bincount(ind, minlength=n).max() <= per_column


def _built_with_image(hip_ops, monkeypatch, m):
    """m.build() with the host copy [n x n] of the image its knn_gram call returned."""
    images, gram = [], hip_ops.knn_gram

    def recording(A):
        images.append(gram(A))
        return images[-1]
    monkeypatch.setattr(hip_ops, 'knn_gram', recording)
    m.build()
    monkeypatch.undo()
    assert len(images) == 1
    n = images[0].shape[0]
    return np.ascontiguousarray(hip_ops.to_host(images[0])[:, :n])


KNN_SETTINGS = [dict(similarity='cosine', neighbours=10), dict(similarity='cosine', neighbours=25, shrink=5.0, normalize=True),
                dict(similarity='cosine', neighbours=10, asymmetric_alpha=0.3), dict(similarity='jaccard', neighbours=10),
                dict(similarity='jaccard', neighbours=40, shrink=2.0, normalize=True)]
RP3_SETTINGS = [dict(neighbours=10), dict(neighbours=25, alpha=0.7, beta=0.4), dict(neighbours=10, beta=0.0, normalize=True),
                dict(neighbours=40, alpha=0.7, beta=0.0)]


def _knn_reference(G, s):
    return ref.item_knn_weights(G, s['similarity'], s['neighbours'], s.get('shrink', 0.0), s.get('asymmetric_alpha', 0.5),
                                s.get('normalize', False))


@pytest.mark.parametrize('name,implicit', [('small', False), ('small', True), ('medium', False), ('synthetic', False)])
def test_item_knn_weights_are_the_restatement(name, implicit, hip_ops, monkeypatch):
    idx, val, shape, A = _case(name, implicit)
    n = shape[1]
    for s in KNN_SETTINGS:
        m = model('ItemKNNModel', hip_ops, idx, val, shape, implicit=implicit, **s)
        G = _built_with_image(hip_ops, monkeypatch, m)
        assert np.array_equal(G, ref.gram(A))                                           # integer feedback: exact
        arrays = _csr_arrays(hip_ops, m.item_weights)
        _same_csr(arrays, _knn_reference(G, s))
        _is_canonical(arrays, n, per_column=s['neighbours'])
        st = m.build_stats
        assert {'gram_s', 'prune_s', 'transpose_s', 'nnz', 'image_bytes', 'neighbours', 'n_items'} <= set(st)
        assert (st['nnz'], st['neighbours'], st['n_items']) == (len(arrays[1]), s['neighbours'], n) and st['transpose_s'] > 0
        assert st['image_bytes'] == n * (-(-n // 8) * 8) * 8 and m.item_weights.nnz == len(arrays[1]) > 0


@pytest.mark.parametrize('name,implicit', [('small', False), ('small', True), ('medium', False), ('synthetic', False)])
def test_rp3_weights_are_the_restatement(name, implicit, hip_ops, monkeypatch):
    idx, val, shape, A = _case(name, implicit)
    n = shape[1]
    for s in RP3_SETTINGS:
        m = model('RP3BetaModel', hip_ops, idx, val, shape, implicit=implicit, **s)
        G = _built_with_image(hip_ops, monkeypatch, m)
        arrays = _csr_arrays(hip_ops, m.item_weights)
        want = ref.rp3_weights(G, A, s.get('alpha', 1.0), s.get('beta', 0.6), s['neighbours'], s.get('normalize', False))
        _same_csr(arrays, want)
        _is_canonical(arrays, n, per_row=s['neighbours'])
        assert (arrays[2] > 0).all() and m.build_stats['transpose_s'] == 0.0 and m.build_stats['nnz'] == want.nnz > 0
        if s.get('normalize'):
            sums = np.add.reduceat(arrays[2], arrays[0][:-1][np.diff(arrays[0]) > 0])
            assert np.allclose(sums, 1.0, rtol=1e-13, atol=0)


def test_unpruned_cosine_is_the_cosine_matrix(hip_ops):
    """neighbours >= n_items - 1, no shrinkage, no normalisation: nothing is pruned."""
    idx, val, shape, A = _case('small')
    n = shape[1]
    m = model('ItemKNNModel', hip_ops, idx, val, shape, neighbours=n - 1)
    m.build()
    G = ref.gram(A)
    norm = np.sqrt(np.diagonal(G))
    want = G / (norm[:, None] * norm[None, :] + 0.0)
    np.fill_diagonal(want, 0.0)
    W = sps.csr_matrix((hip_ops.to_host(m.item_weights.values),) + tuple(hip_ops.to_host(x) for x in
                       (m.item_weights.indices, m.item_weights.indptr)), shape=(n, n)).toarray()
    assert np.array_equal(W, want) and np.array_equal(W, W.T) and (W != 0).sum() > n


@functools.lru_cache(maxsize=None)
def _dyadic():
    """Feedback 1 and users of exactly 4 or 16 items: d_u^(-1/2) is 1/2 or 1/4, every product and partial sum of the Gram
    image of X' is exact, so the image — an fp64 sum whose order the build does not fix — is the same bits in every build."""
    rng = np.random.default_rng(23)
    n_users, n_items = 400, 150
    idx = np.concatenate([np.stack([np.full(k, u), np.sort(rng.choice(n_items, k, replace=False))], 1)
                          for u, k in enumerate(rng.choice([4, 16], n_users))]).astype(np.int64)
    return idx, np.ones(len(idx)), (n_users, n_items)


def test_p3alpha_is_rp3beta_without_the_discount(hip_ops):
    idx, val, shape = _dyadic()
    p = model('P3AlphaModel', hip_ops, idx, val, shape, neighbours=20)
    r = model('RP3BetaModel', hip_ops, idx, val, shape, neighbours=20, beta=0.0)
    b = model('RP3BetaModel', hip_ops, idx, val, shape, neighbours=20)
    for m in (p, r, b):
        m.build()
    pa, ra, ba = (_csr_arrays(hip_ops, m.item_weights) for m in (p, r, b))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(pa, ra))
    assert not np.array_equal(pa[2], ba[2]) and p.method == 'P3alpha'
    A = ref.training_matrix(idx, val, shape)
    _same_csr(pa, ref.rp3_weights(ref.gram(ref.rp3_parts(A, 1.0, 0.0)[0]), A, 1.0, 0.0, 20))


def test_data_objects_that_hand_out_a_stacked_index(hip_ops, monkeypatch):
    """A data object with its own `to_coo` (the protocol of the reference's RecommenderData) builds the restatement's
    weights too."""
    from conftest import GoldenData
    import polara_amd
    idx, val, shape, A = _case('small')
    g = dict(train_idx=idx, train_val=val, train_shape=np.array(shape))
    for name in ('ItemKNNModel', 'RP3BetaModel'):
        m = getattr(polara_amd, name)(GoldenData(g), ops=hip_ops)
        m.verbose = False
        m.neighbours = 10
        G = _built_with_image(hip_ops, monkeypatch, m)
        want = _knn_reference(G, KNN_SETTINGS[0]) if name == 'ItemKNNModel' else ref.rp3_weights(G, A, 1.0, 0.6, 10)
        _same_csr(_csr_arrays(hip_ops, m.item_weights), want)


@pytest.mark.parametrize('cls,settings', [('ItemKNNModel', dict(neighbours=10)), ('ItemKNNModel', dict(similarity='jaccard', neighbours=30, normalize=True)),
                                          ('RP3BetaModel', dict(neighbours=10)), ('RP3BetaModel', dict(neighbours=30, alpha=0.7, normalize=True))])
@pytest.mark.parametrize('implicit', [False, True])
def test_model_lists_scores_and_slices(cls, settings, implicit, hip_ops):
    """Warm start over the fixture's test rows: lists and their scores are SciPy's T.dot(W) over the model's own weights
    followed by the layer's order, in both branches of `dense_output`, with and without `filter_seen`."""
    idx, val, shape, A = _case('medium', implicit)
    test, holdout, tshape = ref.test_rows('medium')
    m = model(cls, hip_ops, idx, val, shape, test, holdout, implicit=implicit, **settings)
    m.build()
    ptr, ind, dat = _csr_arrays(hip_ops, m.item_weights)
    W = sps.csr_matrix((dat, ind, ptr), shape=(shape[1], shape[1]))
    T, seen = i2i_ref.test_matrix(test, tshape, implicit)
    scores = ref.scores(W, T)
    assert not scores[-1].any() and not scores[1].any() and seen[1].any()       # an empty row and a zero-feedback row
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
                assert np.array_equal(list_scores, s_ref), (dense_output, filter_seen, topk)
    assert len(m.training_time) == 1                                            # none of this rebuilt the model
    test_data, test_shape, _ = m._get_test_data()
    block, triplet = m.slice_recommendations(test_data, test_shape, 3, 17)      # the sparse branch: a SciPy CSR
    assert sps.issparse(block) and block.shape == (14, shape[1])
    assert np.array_equal(block.toarray(), scores[3:17]) and (block.data != 0).all()
    m.dense_output = True
    block, triplet = m.slice_recommendations(test_data, test_shape, 3, 17)
    assert isinstance(block, np.ndarray) and np.array_equal(block, scores[3:17])
    assert np.array_equal(triplet[1], test[1][(test[0] >= 3) & (test[0] < 17)])


def test_item_knn_lifecycle(hip_ops):
    idx, val, shape, _ = _case('medium')
    test, holdout, tshape = ref.test_rows('medium')
    m = model('ItemKNNModel', hip_ops, idx, val, shape, test, holdout, neighbours=20)
    m.topk = 10
    recs = m.recommendations
    first = _csr_arrays(hip_ops, m.item_weights)
    assert recs.shape == (tshape[0], 10) and len(m.training_time) == 1
    m.similarity, m.neighbours, m.shrink, m.asymmetric_alpha, m.normalize, m.implicit = 'cosine', 20, 0, 0.5, False, False
    assert m.recommendations is recs and m._is_ready and len(m.training_time) == 1          # unchanged: nothing happens
    W = m.item_weights
    m.dense_output = False                                      # the other branch: new lists, the same model
    assert m.recommendations.shape == recs.shape and m.item_weights is W and len(m.training_time) == 1
    m.dense_output = True
    builds = 1
    for name, value in (('similarity', 'jaccard'), ('neighbours', 7), ('shrink', 3.0), ('asymmetric_alpha', 0.2),
                        ('normalize', True), ('implicit', True)):
        setattr(m, name, value)                                 # a change: the weights are dropped at once, then rebuilt
        assert m.item_weights is None and not m._is_ready, name
        other = m.recommendations
        builds += 1
        assert len(m.training_time) == builds and m.item_weights is not None and other.shape == recs.shape
    m.similarity, m.neighbours, m.shrink, m.asymmetric_alpha, m.normalize, m.implicit = 'cosine', 20, 0, 0.5, False, False
    assert np.array_equal(m.recommendations, recs)
    again = _csr_arrays(hip_ops, m.item_weights)                # the first settings again: the first weights, bit for bit
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, again))
    assert m.evaluate(topk=10) is not None
    m.data.set_training_data((idx[:, 0], idx[:, 1], val * 2))    # a data change: a new model
    assert m.item_weights is None and not m._is_ready


def test_rp3_lifecycle(hip_ops):
    """On the dyadic case (its Gram image is exact, see `_dyadic`): every setting drops the weights, and the first
    settings again give the first weights bit for bit."""
    idx, val, shape = _dyadic()
    m = model('RP3BetaModel', hip_ops, idx, val, shape, neighbours=20)
    m.build()
    first = _csr_arrays(hip_ops, m.item_weights)
    m.alpha, m.beta, m.neighbours, m.normalize = 1, 0.6, 20, False
    assert m._is_ready and m.item_weights is not None and len(m.training_time) == 1
    for builds, (name, value) in enumerate((('alpha', 0.7), ('beta', 0.1), ('neighbours', 5), ('normalize', True)), 2):
        setattr(m, name, value)
        assert m.item_weights is None and not m._is_ready, name
        m.build()
        assert len(m.training_time) == builds and m.item_weights.nnz > 0
        assert not np.array_equal(_csr_arrays(hip_ops, m.item_weights)[2], first[2])
    m.alpha, m.beta, m.neighbours, m.normalize = 1.0, 0.6, 20, False
    m.build()
    again = _csr_arrays(hip_ops, m.item_weights)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(first, again))


@pytest.mark.parametrize('cls', ['ItemKNNModel', 'RP3BetaModel'])
def test_stated_limits(cls, hip_ops, monkeypatch):
    from polara_amd import i2i
    pairs, val, (n_users, n_items), hold = limits_case()
    m = model(cls, hip_ops, pairs, val, (n_users, n_items), holdout=hold, neighbours=1024)
    m.topk = 1024
    assert m.recommendations.shape == (n_users, 1024)
    m.topk = 1025
    with pytest.raises(ValueError, match='1024'):
        m.get_recommendations()
    with pytest.raises(ValueError, match='1024'):
        m.recommend_with_scores()
    # the guard speaks before anything is allocated: a fake free-bytes figure, not an exhausted device
    need = i2i.build_image_bytes(n_items)
    monkeypatch.setattr(hip_ops, 'free_bytes', lambda: 2 * need - 16)
    with pytest.raises(MemoryError, match='%.2f GB' % (need / 1e9)):
        m.build()
    assert m.item_weights is None
    monkeypatch.setattr(hip_ops, 'free_bytes', lambda: 2 * need)
    m.build()
    assert m.item_weights is not None
    monkeypatch.undo()
    bad = val.copy()
    bad[[3, 10, 50]] = -1.0
    m = model(cls, hip_ops, pairs, bad, (n_users, n_items), holdout=hold)
    with pytest.raises(ValueError, match='3 of %d' % len(bad)):
        m.build()
    m.implicit = True                                           # the sign of a negative value is negative too
    with pytest.raises(ValueError, match='3 of %d' % len(bad)):
        m.build()
