"""The item similarities built on the device (polara_amd/similarity.py on csrc/spgemm.hip) against the reference's own
matrices of tests/golden/similarity_*.npz, BIT FOR BIT: row pointers, columns and values; the symmetry of the result, the
cross block against the full matrix, the degenerate shapes of `ops.spgemm_csr` against SciPy's product, and
SimilarityAggregation on a device-made S."""
import numpy as np
import pytest
import scipy.sparse as sps

import similarity_reference as res
import sim_reference as sim
from conftest import load_golden

pytestmark = pytest.mark.gpu

PUBLIC_KIND = {'cosine': 'cosine', 'cosine-binary': 'cosine', 'tfidf-cosine': 'tfidf-cosine', 'jaccard': 'jaccard'}


def _wide(kind):
    return load_golden('similarity_wide_' + kind.replace('-', '_'))


def _similarity(F, kind, fill, hip_ops, **kw):
    from polara_amd import similarity as ps
    if kind == 'cosine-binary':
        return ps.cosine_similarity(F, fill_diagonal=fill, assume_binary=True, ops=hip_ops, **kw)
    return ps.similarity(F, kind, fill_diagonal=fill, ops=hip_ops, **kw)


def _assert_same(got, want, what):
    assert sps.issparse(got) and got.format == 'csr' and got.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(got.indptr, want.indptr), what
    assert np.array_equal(got.indices, want.indices), what
    differ = int((got.data.view(np.uint64) != want.data.view(np.uint64)).sum())
    print('%s: %d entries, %d differ in their bits' % (what, want.nnz, differ))
    assert differ == 0, what


@pytest.mark.parametrize('kind', res.KINDS)
def test_wide_is_bit_equal_and_symmetric(kind, hip_ops):
    g = _wide(kind)
    F = res.features(g)
    for fill in (False, True):
        want = res.stored(g, 'fill%d' % fill)
        got = _similarity(F, kind, fill, hip_ops)
        _assert_same(got, want, '%s fill_diagonal=%s' % (kind, fill))
        assert res.same_bits(got, res.canonical(got.T))
        if fill:
            assert np.array_equal(got.diagonal(), np.ones(F.shape[0]))


def test_device_output_and_device_input(hip_ops):
    from polara_amd.ops import DeviceCSR
    g = _wide('cosine')
    F = res.features(g)
    S = _similarity(F, 'cosine', True, hip_ops, device=True)
    assert isinstance(S, DeviceCSR) and S.shape == (F.shape[0], F.shape[0])
    assert S.indptr.dtype.itemsize == 8 and S.indices.dtype.itemsize == 4 and S.values.dtype.itemsize == 8
    want = res.stored(g, 'fill1')
    assert S.nnz == want.nnz and np.array_equal(hip_ops.to_host(S.values).view(np.uint64), want.data.view(np.uint64))
    Fd = hip_ops.csr(F.indptr, F.indices, F.data, F.shape)
    _assert_same(_similarity(Fd, 'cosine', True, hip_ops), want, 'cosine from a DeviceCSR')


@pytest.mark.parametrize('kind', res.KINDS)
def test_cross_block(kind, hip_ops):
    from polara_amd import similarity as ps
    g = load_golden('similarity_cross')
    F_cols, F_rows = res.features(_wide(kind)), res.features(g, 'rows')
    public, binary = PUBLIC_KIND[kind], kind == 'cosine-binary'
    want = res.stored(g, kind)
    got = ps.cross_similarity(F_rows, F_cols, public, assume_binary=binary, ops=hip_ops)
    _assert_same(got, want, 'cross ' + kind)
    # and against the block of the full device matrix over the stacked items
    full = _similarity(sps.vstack([F_cols, F_rows], format='csr'), kind, False, hip_ops)
    n = F_cols.shape[0]
    assert res.same_bits(got, res.canonical(full[n:, :n]))


@pytest.mark.parametrize('name, fill', [('similarity_wj', True), ('similarity_wj_nofill', False)])
def test_weighted_jaccard(name, fill, hip_ops):
    from polara_amd import similarity as ps
    g = load_golden(name)
    F = res.features(g)
    want = res.stored(g, 'S')
    got = ps.jaccard_similarity_weighted(F, fill_diagonal=fill, ops=hip_ops)
    _assert_same(got, want, name)
    assert res.same_bits(got, res.canonical(got.T))
    n = F.shape[0] - int(g['n_cross_rows'])
    block = ps.cross_similarity(F[n:], F[:n], 'jaccard-weighted', ops=hip_ops)
    assert block.nnz > 0 and res.same_bits(block, res.canonical(want[n:, :n]))


def test_weighted_jaccard_small_and_the_role_of_i_and_j(hip_ops):
    from polara_amd import similarity as ps
    g = load_golden('similarity_wj_small')
    F = res.features(g)
    for fill in (False, True):
        _assert_same(ps.jaccard_similarity_weighted(F, fill_diagonal=fill, ops=hip_ops), res.stored(g, 'fill%d' % fill),
                     'wj_small fill_diagonal=%s' % fill)
    i, j = (int(x) for x in g['role_pair'])
    assert 0 <= i < j                     # the fixture holds a pair whose value depends on which item is walked first
    _, rows = res._rows(F)
    mn, mx = res.weighted_pair(rows[i], rows[j])
    mn2, mx2 = res.weighted_pair(rows[j], rows[i])
    S = res.stored(g, 'fill1')
    assert S[i, j] == S[j, i] == mn / mx != mn2 / mx2


# ---- ops.spgemm_csr on degenerate shapes ------------------------------------------------------------------------------
def _random_csr(rng, n_rows, n_cols, per_row, signed=False):
    rows = []
    for _ in range(n_rows):
        k = min(n_cols, int(rng.integers(0, per_row + 1)))
        rows.append(np.sort(rng.choice(n_cols, k, replace=False)))
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])]
    indices = np.concatenate(rows) if indptr[-1] else np.zeros(0, dtype=np.int64)
    data = rng.integers(1, 30, len(indices)) * 0.1
    if signed:
        data = np.where(rng.random(len(indices)) < 0.5, -data, data)
    return sps.csr_matrix((data, indices, indptr), shape=(n_rows, n_cols))


def _degenerate_cases():
    rng = np.random.default_rng(77)
    cases = {'empty': (sps.csr_matrix((9, 40)), sps.csr_matrix((40, 300))),
             'single row': (_random_csr(rng, 1, 50, 50), _random_csr(rng, 50, 3000, 9))}
    for n_cols in (1, 2048, 2049):
        cases['n_cols = %d' % n_cols] = (_random_csr(rng, 30, 60, 12), _random_csr(rng, 60, n_cols, min(n_cols, 40)))
    # cancelling terms: rows 0 and 1 of B are equal, row 0 of L holds +v and -v on them
    B = _random_csr(rng, 40, 2500, 30, signed=True).tolil()
    B[1] = B[0]
    B = sps.csr_matrix(B)
    L = _random_csr(rng, 20, 40, 10, signed=True).tolil()
    L[0] = 0
    L[0, 0], L[0, 1] = 0.7, -0.7
    L = sps.csr_matrix(L)
    L.eliminate_zeros()
    cases['cancelling terms'] = (L, B)
    return cases


@pytest.mark.parametrize('case', ['empty', 'single row', 'n_cols = 1', 'n_cols = 2048', 'n_cols = 2049', 'cancelling terms'])
def test_spgemm_equals_scipy_on_degenerate_shapes(case, hip_ops):
    L, B = _degenerate_cases()[case]
    L.sort_indices(), B.sort_indices()
    want = res.canonical(L.dot(B))
    if case == 'cancelling terms':
        assert B[0].nnz > 0 and L[0].nnz == 2
        # SciPy on the CPU: the pattern product has entries in row 0, the numeric one drops them all
        assert sps.csr_matrix(abs(L)).dot(sps.csr_matrix(abs(B)))[0].nnz > 0 and want[0].nnz == 0 and want.nnz > 0
    if case == 'empty':
        assert want.nnz == 0
    Ld = hip_ops.csr(L.indptr, L.indices, L.data, L.shape)
    Bd = hip_ops.csr(B.indptr, B.indices, B.data, B.shape)
    C = hip_ops.spgemm_csr(Ld, Bd)
    got = sps.csr_matrix((hip_ops.to_host(C.values), hip_ops.to_host(C.indices), hip_ops.to_host(C.indptr)), shape=C.shape)
    _assert_same(got, want, case)
    assert C.nnz == want.nnz


def test_spgemm_argument_checks(hip_ops):
    from polara_amd._lib import PolaraHipError
    L, B = _degenerate_cases()['n_cols = 2049']
    Ld = hip_ops.csr(L.indptr, L.indices, L.data, L.shape)
    Bd = hip_ops.csr(B.indptr, B.indices, B.data, B.shape)
    with pytest.raises(PolaraHipError, match='square'):
        hip_ops.spgemm_csr(Ld, Bd, diag=True)
    with pytest.raises(PolaraHipError, match='entry counts'):
        hip_ops.spgemm_csr(Ld, Bd, epilogue='jaccard')
    with pytest.raises(PolaraHipError, match='op = MIN'):
        hip_ops.spgemm_csr(Ld, Bd, epilogue='wjaccard')
    with pytest.raises(ValueError, match='columns'):
        hip_ops.spgemm_csr(Bd, Bd)
    with pytest.raises(ValueError, match='unknown'):
        hip_ops.spgemm_csr(Ld, Bd, op='max')


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_similarity_aggregation_on_a_device_made_similarity(hip_ops):
    """SimilarityAggregation on a device-made cosine S over the `sim_sparse` fixture's data returns the lists of the
    restatement on the host-made S.  (The fixture stores its S, not the features it came from, and the reference's data model
    dropped 88 of the generator's items, so the fixture's own S cannot be rebuilt from features here: the features are
    seeded for the fixture's 1 462 items with make_golden_sim.py's generator, and the reference lists of the fixture are
    replaced by the restatement's on the same S.)"""
    from polara_amd import SimilarityAggregation, similarity as ps
    from conftest import GoldenData
    g = dict(load_golden('sim_sparse').items())
    n = int(g['train_shape'][1])
    rng = np.random.RandomState(2)
    rows = [sorted(int(x) for x in rng.choice(300, rng.randint(1, 4), replace=False)) for _ in range(n)]
    F = sps.csr_matrix((np.ones(sum(len(r) for r in rows)), np.concatenate(rows), np.r_[0, np.cumsum([len(r) for r in rows])]),
                       shape=(n, 300))
    S = ps.cosine_similarity(F, ops=hip_ops)
    assert S.shape == (n, n) and res.same_bits(S, res.cosine(F))
    host = res.cosine(F).tocoo()
    g['s_row'], g['s_col'], g['s_val'] = host.row.astype(np.int32), host.col.astype(np.int32), host.data
    data = GoldenData(g)
    data.item_relations = S
    data.warm_start = bool(g['warm_start'])
    m = SimilarityAggregation(data, ops=hip_ops)
    m.verbose = False
    m.implicit, m.dense_output = bool(g['implicit']), bool(g['dense_output'])
    m.topk, m.filter_seen = int(g['topk']), bool(g['filter_seen'])
    scores, cls, lists = sim.sim_lists(g)
    recs = m.recommendations
    assert recs.shape == g['recs'].shape and (recs >= 0).any()
    assert np.array_equal(recs, lists)
