"""The item similarities without a device: the restatement of tests/similarity_reference.py against the reference's own
matrices (tests/golden/similarity_*.npz) bit for bit, what the fixtures are there for, the host-side vectors of
polara_amd/similarity.py, argument errors, kind names, the ABI symbols and `combine_similarity`."""
import numpy as np
import pytest
import scipy.sparse as sps

import similarity_reference as res
from conftest import load_golden


def _wide(kind):
    return load_golden('similarity_wide_' + kind.replace('-', '_'))


@pytest.mark.parametrize('kind', res.KINDS)
def test_restatement_is_bit_equal_to_the_wide_fixtures(kind):
    g = _wide(kind)
    F = res.features(g)
    for fill in (False, True):
        want = res.stored(g, 'fill%d' % fill)
        assert res.same_bits(res.similarity(F, kind, fill), want), (kind, fill)
        assert res.same_bits(want, res.canonical(want.T))
        assert np.isfinite(want.data).all()


@pytest.mark.parametrize('kind', res.KINDS)
def test_restatement_is_bit_equal_to_the_cross_fixture(kind):
    g = load_golden('similarity_cross')
    want = res.stored(g, kind)
    assert want.shape == (70, 2597) and want.nnz > 0
    assert res.same_bits(res.cross(res.features(g, 'rows'), res.features(_wide(kind)), kind), want)


def test_jaccard_fixture_pins_the_boolean_product_of_the_installed_scipy():
    g = _wide('jaccard')
    F = res.features(g)
    for fill in (False, True):
        counted, as_run = res.stored(g, 'fill%d' % fill), g['fill%d_data_as_run' % fill]
        assert len(as_run) == counted.nnz and not np.array_equal(as_run, counted.data)
        # as the reference runs, every intersection counts 1: the value of a pair is 1 / (nf_i + nf_j - 1)
        nf = (F != 0).getnnz(axis=1).astype(np.float64)
        rows = np.repeat(np.arange(F.shape[0]), np.diff(counted.indptr))
        off = rows != counted.indices
        assert np.array_equal(as_run[off], 1.0 / ((nf[rows] + nf[counted.indices]) - 1.0)[off])
        # counted: |i and j| / |i or j| on the dense pattern
    P = (F != 0).astype(np.float64).toarray()
    inter = P @ P.T
    union = nf[:, None] + nf[None, :] - inter
    S = res.stored(g, 'fill0').toarray()
    with np.errstate(invalid='ignore', divide='ignore'):
        assert np.array_equal(S, np.where(inter > 0, inter / union, 0.0))


def test_wide_fixtures_hold_their_cases():
    g = _wide('cosine')
    F = res.features(g)
    assert F.shape == (2597, 600) and F.has_sorted_indices
    per_item, per_label = F.getnnz(axis=1), F.getnnz(axis=0)
    assert (per_item == 0).sum() == 5 and per_item.max() == 130 and per_label.max() == 300
    assert sorted(set(per_item.tolist()) - {0, 130}) == [1, 2, 3, 4]
    assert (F.data == 0).sum() == 2 and 0.15 < (F.data > 1).mean() < 0.25
    long_label = sps.csc_matrix(F)[:, int(per_label.argmax())].indices
    assert long_label.min() < 2048 <= long_label.max()                  # the long row of F^T crosses both windows
    for kind in res.KINDS:
        for fill in (False, True):
            S = res.stored(_wide(kind), 'fill%d' % fill)
            for lo, hi in ((0, 512), (512, 1024), (1536, 2048), (2048, 2597)):
                assert ((S.indices >= lo) & (S.indices < hi)).any()
            empty = np.flatnonzero(per_item == 0)
            assert np.array_equal(np.diff(S.indptr)[empty], np.full(5, int(fill)))     # an all-zero row, a 1 under fill_diagonal
    S0, S1 = (res.stored(g, 'fill%d' % f) for f in (0, 1))
    assert np.array_equal(S1.diagonal(), np.ones(2597)) and not np.array_equal(S0.diagonal(), np.ones(2597))


def test_weighted_jaccard_restatement_and_the_role_of_i_and_j():
    g = load_golden('similarity_wj_small')
    F = res.features(g)
    for fill in (False, True):
        want = res.stored(g, 'fill%d' % fill)
        assert res.same_bits(res.jaccard_weighted(F, fill), want)
        assert res.same_bits(want, res.canonical(want.T))
    # fill_diagonal=False: 1 where the row has labels, not stored otherwise
    d = res.stored(g, 'fill0')
    has = F.getnnz(axis=1) > 0
    assert not has.all() and np.array_equal(d.diagonal(), has.astype(np.float64))
    assert np.array_equal(np.diff(d.indptr)[~has], np.zeros((~has).sum(), dtype=np.diff(d.indptr).dtype))
    i, j = (int(x) for x in g['role_pair'])
    assert 0 <= i < j
    _, rows = res._rows(F)
    mn, mx = res.weighted_pair(rows[i], rows[j])
    mn2, mx2 = res.weighted_pair(rows[j], rows[i])
    assert mn == mn2 and mn / mx != mn2 / mx2 and abs(mn / mx - mn2 / mx2) < 1e-15
    assert want[i, j] == want[j, i] == mn / mx


@pytest.mark.parametrize('name, fill', [('similarity_wj', True), ('similarity_wj_nofill', False)])
def test_weighted_jaccard_large_fixture(name, fill):
    g = load_golden(name)
    F, S = res.features(g), res.stored(g, 'S')
    assert F.shape[0] == 2100 and bool(g['fill_diagonal']) == fill
    for lo, hi in ((0, 512), (512, 1024), (1536, 2048), (2048, 2100)):
        assert ((S.indices >= lo) & (S.indices < hi)).any()
    assert res.same_bits(S, res.canonical(S.T)) and np.isfinite(S.data).all()
    assert res.same_bits(res.jaccard_weighted(F, fill), S)
    n = 2100 - int(g['n_cross_rows'])
    assert res.same_bits(res.cross(F[n:], F[:n], 'jaccard-weighted'), res.canonical(S[n:, :n]))


# ---- the host side of polara_amd/similarity.py ------------------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError('the device backend was touched (%s)' % name)


def test_host_vectors_equal_the_restatement():
    from polara_amd import similarity as ps
    F = res.features(_wide('cosine'))
    sq = np.asarray(F.power(2).sum(axis=1)).reshape(-1)
    assert np.array_equal(ps.safe_inverse_root(sq), res.inverse_root(sq)) 
    assert (ps.safe_inverse_root(sq) == 0).sum() == (sq == 0).sum() >= 5      # items without labels (or with a stored 0 only)
    assert np.array_equal(ps._idf(F), np.log((1 + F.shape[0]) / (1 + F.getnnz(axis=0))))
    indptr, indices, data = ps._reversed_rows(F)
    Fn = res.normalized(F)                      # SciPy emits the rows of diags(norm).dot(F) in reverse: the order of the sums
    keep = data != 0
    rows = np.repeat(np.arange(F.shape[0]), np.diff(indptr))
    keep &= ps.safe_inverse_root(sq)[rows] > 0
    assert np.array_equal(indices[keep], Fn.indices)
    assert np.array_equal((ps.safe_inverse_root(sq)[rows] * data)[keep], Fn.data)
    P = ps._pattern(F)
    assert P.nnz == F.nnz - 2 and (P.data == 1).all() and F.nnz == res.features(_wide('cosine')).nnz


def test_argument_errors_and_kind_names():
    import polara_amd
    from polara_amd import similarity as ps
    assert ps.KINDS == ('jaccard', 'cosine', 'tfidf-cosine', 'jaccard-weighted')
    assert {'cosine_similarity', 'cosine_tfidf_similarity', 'jaccard_similarity', 'jaccard_similarity_weighted',
            'cross_similarity', 'combine_similarity'} <= set(polara_amd.__all__)
    assert polara_amd.cosine_similarity is ps.cosine_similarity
    F = sps.csr_matrix(np.eye(3))
    no = _NoDevice()
    for kind in ('common', 'Cosine ', None):
        with pytest.raises(NotImplementedError, match='kind'):
            ps.similarity(F, kind, ops=no)
    with pytest.raises(NotImplementedError, match="'dice'"):
        ps.cross_similarity(F, F, 'dice', ops=no)
    with pytest.raises(ValueError, match='2-D'):
        ps.cosine_similarity(np.ones(4), ops=no)
    with pytest.raises(ValueError, match='2-D'):
        ps.jaccard_similarity(np.ones((2, 2, 2)), ops=no)
    bad = F.copy()
    bad.data[1] = np.inf
    for fn in (ps.cosine_similarity, ps.cosine_tfidf_similarity, ps.jaccard_similarity, ps.jaccard_similarity_weighted):
        with pytest.raises(ValueError, match='non-finite'):
            fn(bad, ops=no)
    bad.data[1] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        ps.cross_similarity(F, bad, 'cosine', ops=no)
    with pytest.raises(ValueError, match='labels'):
        ps.cross_similarity(F, sps.csr_matrix(np.eye(4)), 'cosine', ops=no)


def test_abi_symbols():
    import re
    import os
    from polara_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'polara_hip.h')).read()
    for name in ('pk_spgemm_work_bytes', 'pk_spgemm_count', 'pk_spgemm_fill'):
        assert name in _lib.PROTOTYPES and re.search(r'\b%s\(' % name, header)
    lib = _lib.load()
    win = lib.pk_i2i_window()
    for n_rows, n_cols in [(0, 1), (1, 1), (30, 2048), (30, 2049), (26744, 26744)]:
        cells = n_rows * -(-n_cols // win)
        al = lambda b: -(-b // 256) * 256
        assert lib.pk_spgemm_work_bytes(n_rows, n_cols) == al(cells * 4) + al((cells + 1) * 8) + al(lib.pk_scan_work_bytes(cells)) + 256
    assert lib.pk_spgemm_work_bytes(3, 0) == -1


def test_combine_similarity_by_hand():
    from polara_amd import similarity as ps
    A = sps.csr_matrix(np.array([[1.0, 0.5, 0.0], [0.5, 1.0, 0.25], [0.0, 0.25, 1.0]]))
    B = sps.csc_matrix(np.array([[0.0, 1.0, 0.5], [1.0, 0.0, 0.0], [0.5, 0.0, 0.0]]))
    S = ps.combine_similarity([A, B])                                    # equal weights 1 / 2
    assert S.format == 'csc' and S.shape == (3, 3)
    assert np.array_equal(S.toarray(), np.array([[1.0, 0.75, 0.25], [0.75, 1.0, 0.125], [0.25, 0.125, 1.0]]))
    S = ps.combine_similarity({'a': A, 'b': B}, {'a': 1.0, 'b': 2.0})    # 0.5 + 2 * 1 = 2.5 is clipped to 1
    assert np.array_equal(S.toarray(), np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 0.25], [1.0, 0.25, 1.0]]))
    assert np.array_equal(S.diagonal(), np.ones(3))
    with pytest.raises(ValueError, match='weights'):
        ps.combine_similarity([A, B], [1.0])
    with pytest.raises(ValueError, match='no matrices'):
        ps.combine_similarity([])
    with pytest.raises(ValueError, match='one shape'):
        ps.combine_similarity([A, sps.csr_matrix(np.eye(4))])
