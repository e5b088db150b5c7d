"""UserKNN and the sparse neighbour pass, host side (no GPU): exports, setting checks and renewal, the argument checks of
pk_spsp_knn_f64 and pk_spsp_topk_seen (which run before any device work), and the NumPy restatement of the pass
(tests/uknn_reference.py) against an independent dense formula and against np.lexsort on ties."""
import numpy as np
import pytest
import scipy.sparse as sps

import uknn_reference as ref

U = ref.U


def _tiny_data():
    from polara_amd.data import ArrayData
    u, i, v = np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([1.0, 2.0, 3.0])
    return ArrayData((u, i, v), n_users=2, n_items=2)


# ---- exports and settings ----------------------------------------------------------------------------------------------
def test_exports_and_defaults():
    import polara_amd
    from polara_amd import knn
    from polara_amd.models import _ItemWeightModel
    assert 'UserKNNModel' in polara_amd.__all__ and polara_amd.UserKNNModel is knn.UserKNNModel
    assert issubclass(knn.UserKNNModel, _ItemWeightModel) and not issubclass(knn.UserKNNModel, knn._PrunedItemModel)
    m = knn.UserKNNModel(_tiny_data())
    assert (m.method, m.similarity, m.neighbours, m.shrink, m.asymmetric_alpha, m.normalize) == ('UserKNN', 'cosine', 100, 0.0, 0.5, False)
    assert (m.implicit, m.dense_output, m._topk_limit) == (False, True, 1024) and m.user_weights is None and m._operand() is None
    assert not hasattr(m, 'item_weights') and not hasattr(m, 'gram')
    for cls in (knn.ItemKNNModel, knn.RP3BetaModel, knn.P3AlphaModel):
        assert cls(_tiny_data()).gram == 'image' and knn.GRAMS == ('image', 'sparse')


def test_bad_settings_raise():
    from polara_amd import knn
    m = knn.UserKNNModel(_tiny_data())
    for bad in ('dice', 'Cosine', None, 1):
        with pytest.raises(ValueError, match='similarity'):
            m.similarity = bad
    for bad in (0, -1, 1025, 2.5):
        with pytest.raises(ValueError, match='neighbours'):
            m.neighbours = bad
    m.neighbours = 1024
    m.neighbours = 1
    for name in ('shrink', 'asymmetric_alpha'):
        for bad in (-1.0, -1e-300, float('nan'), float('inf'), -float('inf')):
            with pytest.raises(ValueError, match=name):
                setattr(m, name, bad)
        setattr(m, name, 0)
        assert getattr(m, name) == 0.0
    with pytest.raises(ValueError, match='asymmetric_alpha'):
        m.asymmetric_alpha = 1.5
    for bad in ('no', 'yes', 2, None, 0.5):
        with pytest.raises(ValueError, match='normalize'):
            m.normalize = bad
    m.normalize = 1
    assert m.normalize is True
    for cls in (knn.ItemKNNModel, knn.RP3BetaModel, knn.P3AlphaModel):
        k = cls(_tiny_data())
        for bad in ('dense', 'Image', None, 0, True):
            with pytest.raises(ValueError, match='gram'):
                k.gram = bad
        k.gram = 'sparse'
        assert k.gram == 'sparse'


def test_each_setting_renews_the_model():
    from polara_amd import knn
    m = knn.UserKNNModel(_tiny_data())
    slots = m._weight_slots
    assert slots == ('_N', '_X', '_Xt', '_q')

    def arm():
        m._is_ready, m._recommendations = True, object()
        for s in slots:
            setattr(m, s, object())

    def held():
        return [getattr(m, s) is not None for s in slots]
    settings = (('similarity', 'jaccard'), ('neighbours', 7), ('shrink', 2.0), ('asymmetric_alpha', 0.3), ('normalize', True),
                ('implicit', True))
    arm()
    for name, _ in settings:
        setattr(m, name, getattr(m, name))                 # unchanged: nothing happens
    assert m._is_ready and all(held()) and m._recommendations is not None
    for name, value in settings:
        arm()
        setattr(m, name, value)
        assert not m._is_ready and not any(held()) and m._recommendations is None, name
    arm()
    m.dense_output = not m.dense_output                    # new lists, the same model
    assert m._is_ready and all(held()) and m._recommendations is None
    arm()
    m.filter_seen = not m.filter_seen
    assert m._is_ready and all(held()) and m._recommendations is None
    for cls in (knn.ItemKNNModel, knn.RP3BetaModel, knn.P3AlphaModel):
        k = cls(_tiny_data())
        k._is_ready, k._W, k._recommendations = True, object(), object()
        k.gram = 'image'
        assert k._is_ready and k._W is not None
        k.gram = 'sparse'
        assert not k._is_ready and k._W is None and k._recommendations is None


def test_multi_process_raises():
    from polara_amd import knn

    class TwoRanks:
        world, rank = 2, 0
    with pytest.raises(NotImplementedError):
        knn.UserKNNModel(_tiny_data(), comm=TwoRanks()).build()


# ---- the library's argument checks -------------------------------------------------------------------------------------
def test_the_neighbour_pass_checks_its_arguments_without_a_device():
    from polara_amd import _lib
    lib = _lib.load()
    p = 4096                                                    # any non-NULL address: every case fails before it is read
    good = dict(n_rows=10, n_inner=7, n_cols=12, l_indptr=p, l_indices=p, l_values=p, l_kind=1, b_indptr=p, b_indices=p,
                b_values=p, kind=1, row=p, col=p, shrink=0.0, exclude=None, K=5, normalize=0, count=p, idx=p, val=p, work=p)

    def call(**changed):
        a = dict(good, **changed)
        return lib.pk_spsp_knn_f64(None, *(a[k] for k in good))
    bad = [(dict(n_rows=-1), b'shape'), (dict(n_inner=0), b'shape'), (dict(n_cols=0), b'shape'), (dict(n_cols=2 ** 30), b'shape'),
           (dict(l_kind=2), b'value kind'), (dict(kind=3), b'kind'), (dict(kind=-1), b'kind'), (dict(K=0), b'K ='),
           (dict(K=1025), b'K ='), (dict(shrink=-1e-300), b'shrink'), (dict(shrink=float('nan')), b'shrink'),
           (dict(shrink=float('inf')), b'shrink')]
    bad += [({name: None}, b'null') for name in ('l_indptr', 'b_indptr', 'row', 'col', 'count', 'idx', 'val', 'work')]
    for changed, word in bad:
        assert call(**changed) == -1, changed                   # PK_E_INVALID
        message = lib.pk_last_error()
        assert message.startswith(b'pk_spsp_knn_f64') and word in message, (changed, message)
    assert call(n_rows=0) == 0                                  # nothing to do: no launch
    # the scratch: the candidate keys of pk_spsp_topk for one chunk of rows plus the chunk's merged lists (16 bytes a slot)
    for n_rows, n_cols, K in ((10, 12, 5), (14600, 4097, 1024), (3000, 3000, 100)):
        chunk = lib.pk_i2i_chunk_users(n_rows, n_cols, K)
        base = lib.pk_spsp_topk_work_bytes(n_rows, n_cols, K)
        assert lib.pk_spsp_knn_work_bytes(n_rows, n_cols, K) == -(-base // 8) * 8 + chunk * K * 16
    assert lib.pk_i2i_chunk_users(14600, 4097, 1024) == 14563   # the chunked case of the device tests: two chunks
    assert lib.pk_spsp_knn_work_bytes(10, 12, 0) == 0 and lib.pk_spsp_knn_work_bytes(10, 12, 1025) == 0


def test_topk_seen_checks_its_arguments_without_a_device():
    from polara_amd import _lib
    lib = _lib.load()
    p = 4096
    good = dict(n_rows=10, n_inner=7, n_cols=12, l_indptr=p, l_indices=p, l_values=p, l_kind=1, b_indptr=p, b_indices=p,
                b_values=p, s_indptr=p, s_indices=p, topk=5, filter_seen=1, sparse=0, out=p, scores=None, work=p)

    def call(**changed):
        a = dict(good, **changed)
        return lib.pk_spsp_topk_seen(None, *(a[k] for k in good))
    bad = [(dict(topk=0), b'topk'), (dict(topk=1025), b'topk'), (dict(n_cols=0), b'shape'), (dict(n_inner=0), b'shape'),
           (dict(l_kind=5), b'value kind'), (dict(l_indptr=None), b'null'), (dict(b_indptr=None), b'null'),
           (dict(s_indptr=None), b'null'), (dict(out=None), b'null'), (dict(work=None), b'null')]
    for changed, word in bad:
        assert call(**changed) == -1, changed
        message = lib.pk_last_error()
        assert message.startswith(b'pk_spsp_topk_seen') and word in message, (changed, message)
    assert call(n_rows=0) == 0
    # pk_spsp_topk keeps its own check: its seen set is the left row, so the inner dimension must be the catalogue
    assert lib.pk_spsp_topk(None, 10, 7, 12, p, p, p, 1, p, p, p, 5, 1, 0, p, None, p) == -1
    assert b'n_inner == n_cols' in lib.pk_last_error()


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _integer_matrix():
    """40 users x 25 items, feedback 1..5, an item and a user without entries."""
    rng = np.random.default_rng(11)
    X = np.where(rng.random((40, 25)) < 0.4, rng.integers(1, 6, (40, 25)), 0).astype(np.float64)
    X[:, 7] = 0
    X[13] = 0
    return sps.csr_matrix(X)


@pytest.mark.parametrize('similarity,shrink,alpha', [('cosine', 0.0, 0.5), ('cosine', 5.0, 0.5), ('cosine', 0.0, 0.3),
                                                     ('jaccard', 0.0, 0.5), ('jaccard', 5.0, 0.5)])
def test_user_knn_restatement_against_the_textbook(similarity, shrink, alpha):
    """N before pruning (neighbours = n_users - 1 keeps every candidate) within gamma(m) relative, m the longest row of X.
    Derived: g_uv and q_v are sums of at most m products of integers <= 5, exact in fp64 on both sides in any order;
    an entry then takes at most 8 roundings on either side (two powers, a product, two sums, a quotient), and
    8 u <= gamma(m) because the longest row of this matrix holds m >= 8 entries."""
    A = _integer_matrix()
    n = A.shape[0]
    m = int(np.diff(A.indptr).max())
    assert m >= 8
    W = ref.user_knn_weights(A, similarity, n - 1, shrink, alpha).toarray()
    want = ref.textbook_user_knn(A, similarity, shrink, alpha)
    off = ~np.eye(n, dtype=bool)
    want = np.where(np.isfinite(want), want, 0.0)              # 0 / 0 of the empty user: no candidate, no weight
    assert np.array_equal(W[off] != 0, want[off] != 0) and not W[~off].any()
    nz = off & (want != 0)
    gap = float((np.abs(W[nz] - want[nz]) / np.abs(want[nz])).max())
    print('relative gap %.3g u, bound gamma(%d) = %.3g u' % (gap / U, m, ref.gamma(m) / U))
    assert gap <= ref.gamma(m)
    assert not W[13].any() and not W[:, 13].any()              # the empty user neither has nor is a neighbour
    if similarity == 'cosine' and alpha == 0.5 and shrink == 0.0:
        assert np.allclose(W, W.T, rtol=4 * U, atol=0)         # the plain cosine is symmetric


def test_sparse_route_restatement_is_the_image_restatement_on_integers():
    """On integer feedback both Gram matrices are exact, so the sparse-order restatement of ItemKNN and the image-order one
    (tests/knn_reference.py) are the same matrix bit for bit; for RP3beta (X' is not integer) they agree within 2 gamma(m)."""
    import knn_reference as knn_ref
    A = _integer_matrix()
    G = knn_ref.gram(A)
    for similarity, shrink, alpha, normalize in (('cosine', 0.0, 0.5, False), ('cosine', 3.0, 0.3, True), ('jaccard', 1.0, 0.5, True)):
        a = ref.item_knn_sparse_weights(A, similarity, 6, shrink, alpha, normalize)
        b = knn_ref.item_knn_weights(G, similarity, 6, shrink, alpha, normalize)
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        assert np.array_equal(a.data.view(np.int64), b.data.view(np.int64))
    X = knn_ref.rp3_parts(A, 0.7, 0.4)[0]
    m = int(np.diff(A.tocsc().indptr).max())
    a = ref.rp3_sparse_weights(A, 0.7, 0.4, 24).toarray()      # 24 = n_items - 1: nothing pruned
    b = knn_ref.rp3_weights(knn_ref.gram(X), A, 0.7, 0.4, 24).toarray()
    assert np.array_equal(a != 0, b != 0)
    assert (np.abs(a - b)[b != 0] / b[b != 0]).max() <= 2 * ref.gamma(m)


def test_selection_against_lexsort_on_ties():
    """A rectangular g of few distinct values with an excluded column per row: kept = the first K of lexsort
    (column, -w) over the candidates, written in ascending column order; the absolute sum is the left-to-right one."""
    rng = np.random.default_rng(5)
    n_rows, n_cols = 30, 70
    g = rng.integers(-2, 3, (n_rows, n_cols)).astype(np.float64)
    row, col = rng.integers(1, 3, n_rows).astype(np.float64), rng.integers(1, 3, n_cols).astype(np.float64)
    exclude = rng.integers(0, n_cols, n_rows).astype(np.int32)
    exclude[4] = -1                                            # nothing excluded in this row
    w = (g * row[:, None]) * col[None, :]
    for K in (1, 5, 69, 128):
        for normalize in (False, True):
            count, idx, val = ref.slots(g, ref.SCALE, row, col, 0.0, K, normalize, exclude)
            assert count.dtype == np.int32 and idx.dtype == np.int32 and idx.shape == val.shape == (n_rows, K)
            for i in range(n_rows):
                cand = np.flatnonzero((g[i] != 0) & (np.arange(n_cols) != exclude[i]))
                kept = np.sort(cand[np.lexsort((cand, -w[i, cand]))][:K])
                assert count[i] == len(kept) == min(K, len(cand)) and np.array_equal(idx[i, :count[i]], kept)
                assert (idx[i, count[i]:] == -1).all() and not val[i, count[i]:].any()
                want = w[i, kept]
                if normalize:
                    s = 0.0
                    for x in want:
                        s = s + abs(float(x))
                    want = want / s
                assert np.array_equal(val[i, :count[i]], want)
    free = ref.slots(g, ref.SCALE, row, col, 0.0, 128, False, None)
    assert (free[0] >= count).all() and free[0][4] == count[4] and free[0].sum() > count.sum()
    assert (val < 0).any()


def test_host_vectors_are_the_restatements():
    from polara_amd import knn
    rng = np.random.default_rng(2)
    keys, vals = rng.integers(0, 9, 200), rng.random(200) * 3
    assert np.array_equal(knn.squared_sums(keys, vals, 12), ref.squared_sums(keys, vals, 12))
    q_r, q_c = rng.random(5) * 7, rng.random(8) * 7
    for sim, a in (('cosine', 0.5), ('cosine', 0.3), ('cosine', 1.0), ('jaccard', 0.5)):
        got, want = knn._similarity_vectors(sim, q_r, q_c, a), ref.similarity_vectors(sim, q_r, q_c, a)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert len(got[1]) == 5 and len(got[2]) == 8
