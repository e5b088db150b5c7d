"""ItemKNN and RP3beta, host side (no GPU): exports, setting checks and renewal, the argument checks of pk_knn_prune_f64
(which run before any device work), and the NumPy restatement of the pruning pass (tests/knn_reference.py) against
independent dense formulas and against np.lexsort on ties."""
import numpy as np
import pytest
import scipy.sparse as sps

import knn_reference as ref

U = 2.0 ** -53


def _tiny_data():
    from polara_amd.data import ArrayData
    u, i, v = np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([1.0, 2.0, 3.0])
    return ArrayData((u, i, v), n_users=2, n_items=2)


# ---- exports and settings ----------------------------------------------------------------------------------------------
def test_exports_and_defaults():
    import polara_amd
    from polara_amd import knn
    from polara_amd.models import _ItemWeightModel
    for name in ('ItemKNNModel', 'RP3BetaModel', 'P3AlphaModel'):
        assert name in polara_amd.__all__ and getattr(polara_amd, name) is getattr(knn, name)
        assert issubclass(getattr(knn, name), _ItemWeightModel)
    assert issubclass(knn.P3AlphaModel, knn.RP3BetaModel)
    m = knn.ItemKNNModel(_tiny_data())
    assert (m.method, m.similarity, m.neighbours, m.shrink, m.asymmetric_alpha, m.normalize) == ('ItemKNN', 'cosine', 100, 0.0, 0.5, False)
    assert (m.implicit, m._topk_limit, m._weight_slots) == (False, 1024, ('_W',)) and m.item_weights is None and m._operand() is None
    r = knn.RP3BetaModel(_tiny_data())
    assert (r.method, r.alpha, r.beta, r.neighbours, r.normalize, r._topk_limit) == ('RP3beta', 1.0, 0.6, 100, False, 1024)
    p = knn.P3AlphaModel(_tiny_data())
    assert (p.method, p.alpha, p.beta) == ('P3alpha', 1.0, 0.0)
    p.beta = 0
    with pytest.raises(ValueError, match='beta'):
        p.beta = 0.3


def test_bad_settings_raise():
    from polara_amd import knn
    m, r = knn.ItemKNNModel(_tiny_data()), knn.RP3BetaModel(_tiny_data())
    for bad in ('dice', 'Cosine', None, 1):
        with pytest.raises(ValueError, match='similarity'):
            m.similarity = bad
    for model in (m, r):
        for bad in (0, -1, 1025, 2.5):
            with pytest.raises(ValueError, match='neighbours'):
                model.neighbours = bad
        model.neighbours = 1024
        model.neighbours = 1
    for model, name in ((m, 'shrink'), (m, 'asymmetric_alpha'), (r, 'alpha'), (r, 'beta')):
        for bad in (-1.0, -1e-300, float('nan'), float('inf'), -float('inf')):
            with pytest.raises(ValueError, match=name):
                setattr(model, name, bad)
        setattr(model, name, 0)
        assert getattr(model, name) == 0.0
    with pytest.raises(ValueError, match='asymmetric_alpha'):
        m.asymmetric_alpha = 1.5
    for model in (m, r):
        for bad in ('no', 'yes', 2, None, 0.5):
            with pytest.raises(ValueError, match='normalize'):
                model.normalize = bad
        model.normalize = 1
        assert model.normalize is True
        model.normalize = False
    assert (m.similarity, m.neighbours, r.neighbours) == ('cosine', 1, 1)


def test_each_setting_renews_the_model():
    from polara_amd import knn
    cases = ((knn.ItemKNNModel, (('similarity', 'jaccard'), ('neighbours', 7), ('shrink', 2.0), ('asymmetric_alpha', 0.3),
                                 ('normalize', True), ('implicit', True))),
             (knn.RP3BetaModel, (('alpha', 0.7), ('beta', 0.2), ('neighbours', 7), ('normalize', True), ('implicit', True))),
             (knn.P3AlphaModel, (('alpha', 0.7), ('neighbours', 7))))
    for cls, settings in cases:
        m = cls(_tiny_data())

        def arm():
            m._is_ready, m._W, m._recommendations = True, object(), object()
        arm()
        for name, _ in settings:
            setattr(m, name, getattr(m, name))                 # unchanged: nothing happens
        assert m._is_ready and m._W is not None and m._recommendations is not None
        for name, value in settings:
            arm()
            setattr(m, name, value)
            assert not m._is_ready and m._W is None and m._recommendations is None, (cls.__name__, name)
        arm()
        m.dense_output = not m.dense_output                    # new lists, the same model
        assert m._is_ready and m._W is not None and m._recommendations is None


def test_multi_process_raises():
    from polara_amd import knn

    class TwoRanks:
        world, rank = 2, 0
    for cls in (knn.ItemKNNModel, knn.RP3BetaModel, knn.P3AlphaModel):
        with pytest.raises(NotImplementedError):
            cls(_tiny_data(), comm=TwoRanks()).build()


# ---- the library's argument checks ----------------------------------------------------------------------------------------
def test_the_library_checks_its_arguments_without_a_device():
    from polara_amd import _lib, knn
    lib = _lib.load()
    assert lib.pk_knn_max_neighbours() == knn.MAX_NEIGHBOURS == lib.pk_i2i_max_topk() == 1024
    assert (_lib.PK_KNN_SCALE, _lib.PK_KNN_COSINE, _lib.PK_KNN_TANIMOTO) == (ref.SCALE, ref.COSINE, ref.TANIMOTO) == (0, 1, 2)
    assert knn.KINDS == {'scale': 0, 'cosine': 1, 'tanimoto': 2}
    p = 4096                                                    # any non-NULL address: every case fails before it is read
    good = dict(n=10, G=p, ldg=16, kind=1, row=p, col=p, shrink=0.0, K=5, normalize=0, count=p, idx=p, val=p)

    def call(**changed):
        a = dict(good, **changed)
        return lib.pk_knn_prune_f64(None, a['n'], a['G'], a['ldg'], a['kind'], a['row'], a['col'], a['shrink'], a['K'],
                                    a['normalize'], a['count'], a['idx'], a['val'])
    bad = [(dict(n=0), b'n ='), (dict(n=-3), b'n ='), (dict(n=2 ** 30, ldg=2 ** 30), b'n ='), (dict(ldg=9), b'ldg'),
           (dict(kind=3), b'kind'), (dict(kind=-1), b'kind'), (dict(K=0), b'K ='), (dict(K=1025), b'K ='),
           (dict(shrink=-1e-300), b'shrink'), (dict(shrink=float('nan')), b'shrink'), (dict(shrink=float('inf')), b'shrink')]
    bad += [({name: None}, b'null') for name in ('G', 'row', 'col', 'count', 'idx', 'val')]
    for changed, word in bad:
        assert call(**changed) == -1, changed                   # PK_E_INVALID
        message = lib.pk_last_error()
        assert message.startswith(b'pk_knn_prune_f64') and word in message, (changed, message)


# ---- the restatement -------------------------------------------------------------------------------------------------------
def _integer_matrix():
    """40 x 25, feedback 1..5, an item and a user without entries."""
    rng = np.random.default_rng(11)
    X = np.where(rng.random((40, 25)) < 0.3, rng.integers(1, 6, (40, 25)), 0).astype(np.float64)
    X[:, 7] = 0
    X[13] = 0
    return sps.csr_matrix(X)


def _unpruned(count, idx, val, n):
    W = np.zeros((n, n))
    for i in range(n):
        W[i, idx[i, :count[i]]] = val[i, :count[i]]
    return W


def _relative_gap(W, want):
    off = ~np.eye(len(W), dtype=bool)
    want = np.where(np.isfinite(want), want, 0.0)              # 0 / 0 of the empty item: no candidate, no weight
    assert np.array_equal(W[off] != 0, want[off] != 0) and not W[~off].any()
    nz = off & (want != 0)
    return float((np.abs(W[nz] - want[nz]) / np.abs(want[nz])).max())


@pytest.mark.parametrize('similarity,shrink,alpha', [('cosine', 0.0, 0.5), ('cosine', 5.0, 0.5), ('cosine', 0.0, 0.3),
                                                     ('jaccard', 0.0, 0.5), ('jaccard', 5.0, 0.5)])
def test_item_knn_restatement_against_the_textbook(similarity, shrink, alpha):
    """W before pruning (neighbours = n - 1 keeps every candidate) within 8 u relative: the Gram matrix of integer data
    is exact, an entry then takes a handful of roundings (two powers, a product, a sum, a quotient) on either side."""
    A = _integer_matrix()
    G, n = ref.gram(A), A.shape[1]
    assert np.array_equal(G, np.round(G))
    W = ref.item_knn_weights(G, similarity, n - 1, shrink, alpha).toarray()
    gap = _relative_gap(W, ref.textbook_item_knn(A, similarity, shrink, alpha))
    print('relative gap %.3g u' % (gap / U))
    assert gap <= 8 * U
    assert not W[7].any() and not W[:, 7].any()                # the empty item: 0 / 0 with shrink = 0, g = 0 anyway


@pytest.mark.parametrize('alpha', [1.0, 0.7])
@pytest.mark.parametrize('beta', [0.0, 0.4])
def test_rp3_restatement_against_the_textbook(alpha, beta):
    """r_i G'[i, j] c_j against pop_j^(-beta) sum_u (a_ui / d_i)^alpha (a_uj / d_u)^alpha within 8 u relative, the bound of
    the cosine and Jaccard cases: a handful of roundings per entry on either side (measured: 4.0 to 4.7 u at m = 19)."""
    A = _integer_matrix()
    n = A.shape[1]
    X, r, c = ref.rp3_parts(A, alpha, beta)
    m = int(np.diff(A.tocsc().indptr).max())
    W = _unpruned(*ref.prune(ref.gram(X), ref.SCALE, r, c, 0.0, n - 1, False), n)
    gap = _relative_gap(W, ref.textbook_rp3(A, alpha, beta))
    print('relative gap %.3g u, m = %d' % (gap / U, m))
    assert gap <= 8 * U
    if beta == 0.0:
        assert np.array_equal(c, (np.diff(A.tocsc().indptr) > 0).astype(np.float64))


def test_selection_against_lexsort_on_ties():
    """Few distinct values: most of a row is tied.  Kept = the first K of lexsort (column, -w) over the candidates, written
    in ascending column order; the absolute sum is the left-to-right one."""
    rng = np.random.default_rng(5)
    n = 60
    G = rng.integers(-2, 3, (n, n)).astype(np.float64)         # negative entries, zeros, not symmetric
    row, col = rng.integers(1, 3, n).astype(np.float64), rng.integers(1, 3, n).astype(np.float64)
    w = (G * row[:, None]) * col[None, :]
    for K in (1, 5, 59, 64):
        for normalize in (False, True):
            count, idx, val = ref.prune(G, ref.SCALE, row, col, 0.0, K, normalize)
            assert count.dtype == np.int32 and idx.dtype == np.int32 and idx.shape == val.shape == (n, K)
            for i in range(n):
                cand = np.flatnonzero((G[i] != 0) & (np.arange(n) != i))
                kept = np.sort(cand[np.lexsort((cand, -w[i, cand]))][:K])
                assert count[i] == len(kept) == min(K, len(cand)) and np.array_equal(idx[i, :count[i]], kept)
                assert (idx[i, count[i]:] == -1).all() and not val[i, count[i]:].any()
                want = w[i, kept]
                if normalize:
                    s = 0.0
                    for x in want:
                        s = s + abs(float(x))
                    assert s == ref.sequential_abs_sum(want)
                    want = want / s
                assert np.array_equal(val[i, :count[i]], want)
    assert (val < 0).any() and count.min() < 59                 # negative weights are kept below positive ones when K allows


def test_host_vectors_are_the_restatements():
    from polara_amd import knn
    q = np.array([0.0, 1.0, 2.0, 9.0, 1e-3, 123456.0])
    assert np.array_equal(knn.power(q, 0.5), np.sqrt(q)) and np.array_equal(knn.power(q, 0.3), np.power(q, 0.3))
    for a in (0.5, 0.3, 0.0, 1.0):
        row, col = knn.cosine_vectors(q, a)
        assert np.array_equal(row, ref.power(q, 1.0 - a)) and np.array_equal(col, ref.power(q, a))
    su, r, c = knn.rp3_vectors(q, q[::-1], q, 0.7, 0.4)
    assert np.array_equal(su, ref.inverse_power(q, 0.35)) and np.array_equal(r, ref.inverse_power(q[::-1], 0.7))
    assert np.array_equal(c, ref.inverse_power(q, 0.4)) and su[0] == 0.0 and c[0] == 0.0
    assert np.array_equal(knn.inverse_power(q, 0.0), (q > 0).astype(np.float64))
