"""HybridSVD, host side (no GPU): the NumPy/SciPy restatement (tests/hybrid_reference.py) against the reference's own
fixtures (tests/golden/hybrid_*.npz from tests/golden/make_golden_hybrid.py), SimilarityArrayData, the beta mapping,
the planning and memory guard of polara_amd/hybrid.py (held together with the library's pk_hybrid_* queries), and the
model's orchestration on a CPU double of the device operators."""
import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sps
import torch

import hybrid_reference as ref
from conftest import load_golden
from numpy_ops import NumpyOps

FIXTURES = ['hybrid_known', 'hybrid_nofilter', 'hybrid_warm', 'hybrid_scaled', 'hybrid_weight_02', 'hybrid_weight_09']


class HybridNumpyOps(NumpyOps):
    """The CPU double plus the four HybridSVD operators (image layout as on the device: padded to whole tiles)."""

    def hybrid_densify(self, S, rank, beta):
        from polara_amd import hybrid
        n = S.shape[0]
        ld = hybrid.leading_dim(n)
        K = np.zeros((ld, ld))
        c = sps.tril(sps.csr_matrix(S)[:, np.argsort(rank)][np.argsort(rank), :]).tocoo()
        K[c.row, c.col] = c.data
        K[np.arange(n), np.arange(n)] += beta
        return torch.from_numpy(K)

    def chol(self, A, n):
        K = A.numpy()[:n, :n]
        try:
            L = np.linalg.cholesky(np.tril(K) + np.tril(K, -1).T)
        except np.linalg.LinAlgError:
            d = np.tril(K) + np.tril(K, -1).T
            col = next(j for j in range(1, n + 1) if np.any(np.linalg.eigvalsh(d[:j, :j]) <= 0)) - 1
            err = np.linalg.LinAlgError('not positive definite at column %d' % col)
            err.column = col
            raise err
        A.zero_()
        A[:n, :n] = torch.from_numpy(L)
        A[n:, n:] = torch.eye(A.shape[0] - n, dtype=torch.float64)
        return A

    def trmm(self, L, n, X, trans=False, out=None):
        Lh = L.numpy()[:n, :n]
        Y = torch.from_numpy((Lh.T if trans else Lh) @ X.numpy())
        if out is not None:
            out.copy_(Y)
            return out
        return Y

    def trsm(self, L, n, B):
        B = B.numpy() if isinstance(B, torch.Tensor) else np.asarray(B)
        return torch.from_numpy(scipy.linalg.solve_triangular(L.numpy()[:n, :n], B, lower=True, trans='T'))


def golden_data(g):
    from polara_amd.data import SimilarityArrayData

    class _HD(SimilarityArrayData):
        def __init__(self, g):
            self.g = g
            idx = g['train_idx']
            shp = tuple(int(x) for x in g['train_shape'])
            super().__init__((idx[:, 0], idx[:, 1], g['train_val']), n_users=shp[0], n_items=shp[1],
                             relations_matrices={'itemid': ref.relations(g), 'userid': None},
                             relations_indices={'itemid': None, 'userid': None})
            self.warm_start = bool(g['warm_start'])

        def to_coo(self, tensor_mode=False, feedback_threshold=None):
            g = self.g
            return g['train_idx'].astype(np.intp), g['train_val'], tuple(int(x) for x in g['train_shape'])

        def test_to_coo(self, tensor_mode=False, feedback_threshold=None):
            g = self.g
            return (g['test_user'], g['test_item'], g['test_fdbk'])

        def get_test_shape(self, tensor_mode=False):
            s = tuple(int(x) for x in self.g['test_shape'])
            return s if tensor_mode else s[:2]
    return _HD(g)


def model_for(g, ops, weight=None):
    from polara_amd.models import HybridSVD, ScaledHybridSVD
    cls = ScaledHybridSVD if str(g['model']).endswith('-s') else HybridSVD
    m = cls(golden_data(g), ops=ops)
    m.verbose = False
    m.rank = int(g['rank'])
    m.topk = int(g['topk'])
    m.filter_seen = bool(g['filter_seen'])
    m.features_weight = float(g['features_weight']) if weight is None else weight
    return m


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_matches_the_reference(name):
    g = load_golden(name)
    sigma, vl, vr, scores, cls, lists = ref.fixture_model(g)
    assert np.allclose(sigma, g['sigma'], rtol=1e-10, atol=0)
    assert ref.same_up_to_sign(vl, g['vl'], 1e-8) and ref.same_up_to_sign(vr, g['vr'], 1e-8)
    n = g['scores'].shape[0]
    assert np.allclose(scores[:n], g['scores'], rtol=1e-9, atol=1e-10)
    assert np.array_equal(lists, g['recs'])


def test_fixtures_hold_the_reference_surface():
    g = load_golden('hybrid_scaled')
    assert str(g['model']) == 'HybridSVD-s'
    for name in FIXTURES:
        g = load_golden(name)
        assert int(g['builds_after_rank5']) == 1             # the truncation did not rebuild
        assert g['recs_rank5'].shape == g['recs'].shape


def test_beta_mapping():
    from polara_amd.hybrid import beta_of
    assert beta_of(0.5) == 1.0 and beta_of(1.0) == 0.0
    assert np.isclose(beta_of(0.2), 4.0) and np.isclose(beta_of(0.9), 1.0 / 9.0)
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            beta_of(bad)


def test_planning_matches_the_library():
    from polara_amd import _lib, hybrid
    lib = _lib.load()
    assert lib.pk_hybrid_max_nc() == hybrid.MAX_NC
    for n in (1, 15, 16, 17, 63, 64, 65, 200, 1000, 4099, 26744, 100000):
        assert lib.pk_hybrid_ld(n) == hybrid.leading_dim(n) and hybrid.leading_dim(n) % 64 == 0
        for nc in (1, 16, 64):
            assert lib.pk_trmm_work_bytes(n, nc) == hybrid.trmm_work_bytes(n, nc)
    assert hybrid.image_bytes(26744) == 26752 * 26752 * 8
    assert hybrid.column_blocks(150) == [(0, 64), (64, 128), (128, 150)]


def test_memory_guard():
    from polara_amd import hybrid
    need = hybrid.image_bytes(26744)
    assert hybrid.check_factor_memory(26744, 2 * need) == need
    with pytest.raises(MemoryError, match='Cholesky'):
        hybrid.check_factor_memory(26744, 2 * need - 1)
    with pytest.raises(MemoryError):
        hybrid.check_factor_memory(200000, 288e9)           # 320 GB of fp64 at 200 000 items


def test_similarity_array_data():
    from polara_amd.data import SimilarityArrayData
    rng = np.random.default_rng(0)
    S = sps.random(6, 6, density=0.5, random_state=1, format='csr')
    S = (S + S.T).tocsr()
    diag0 = S.diagonal().copy()
    idx = np.array([5, 3, 1, 0, 2, 4])                   # row r of S belongs to item idx[r]
    d = SimilarityArrayData((np.arange(4), rng.integers(0, 6, 4), np.ones(4)), n_users=4, n_items=6,
                            relations_matrices={'itemid': S, 'userid': None},
                            relations_indices={'itemid': idx, 'userid': None})
    R = d.item_relations.toarray()
    rows = np.argsort(idx)
    expect = S.toarray()[np.ix_(rows, rows)]
    np.fill_diagonal(expect, 1)
    assert np.array_equal(R, expect)
    assert d.user_relations is None
    assert d.get_relations_matrix('itemid') is d.item_relations            # cached
    assert np.array_equal(S.diagonal(), diag0)                              # the caller's matrix is not written
    first = d.item_relations
    d.set_training_data((np.arange(4), rng.integers(0, 6, 4), np.ones(4)))  # a data-change event drops the cache
    assert d.item_relations is not first and np.array_equal(d.item_relations.toarray(), expect)
    dense = SimilarityArrayData((np.arange(4), rng.integers(0, 6, 4), np.ones(4)), n_users=4, n_items=6,
                                relations_matrices={'itemid': S.toarray()}, relations_indices={'itemid': None})
    exp2 = S.toarray().copy()
    np.fill_diagonal(exp2, 1)
    assert np.array_equal(dense.item_relations, exp2)


@pytest.mark.parametrize('name', FIXTURES)
def test_model_orchestration_on_the_cpu_double(name):
    g = load_golden(name)
    m = model_for(g, HybridNumpyOps())
    recs = m.recommendations
    sigma, vl, vr, scores, cls, lists = ref.fixture_model(g)
    assert np.allclose(m.factors['singular_values'], g['sigma'], rtol=1e-8)
    pl, pr = m.get_item_projector()
    assert ref.same_up_to_sign(pl, g['vl'], 1e-7) and ref.same_up_to_sign(pr, g['vr'], 1e-7)
    assert np.array_equal(recs, g['recs'])
    assert m.method == str(g['model'])
    m.rank = 5
    assert np.array_equal(m.recommendations, g['recs_rank5'])
    assert len(m.training_time) == 1


def test_model_errors_and_surface():
    from polara_amd.data import ArrayData, SimilarityArrayData
    from polara_amd.models import HybridSVD
    g = load_golden('hybrid_known')
    ops = HybridNumpyOps()
    idx = g['train_idx']
    train = (idx[:, 0], idx[:, 1], g['train_val'])
    with pytest.raises(ValueError, match='SVDModel'):
        HybridSVD(ArrayData(train), ops=ops).build()
    S = ref.relations(g)
    user_rel = sps.identity(int(g['train_shape'][0]), format='csr')
    d = SimilarityArrayData(train, relations_matrices={'itemid': S, 'userid': user_rel},
                            relations_indices={'itemid': None, 'userid': None})
    with pytest.raises(NotImplementedError):
        HybridSVD(d, ops=ops).build()
    A = S.tolil()
    A[0, 1] = A[1, 0] + 0.5
    d = SimilarityArrayData(train, relations_matrices={'itemid': A.tocsr()}, relations_indices={'itemid': None})
    with pytest.raises(ValueError, match='symmetric'):
        HybridSVD(d, ops=ops).build()
    bad = S.tolil()
    bad[3, 3] = -5.0                                         # K = S + I with a negative pivot at item 3
    d = SimilarityArrayData(train, relations_matrices={'itemid': bad.tocsr()}, relations_indices={'itemid': None})
    d._relations['itemid'] = bad.tocsr()                     # (the diagonal is reset to 1 on load: inject the matrix)
    m = HybridSVD(d, ops=ops)
    with pytest.raises(np.linalg.LinAlgError):
        m.build()

    class World2:
        world, rank = 2, 0
    m = HybridSVD(golden_data(g), ops=ops, comm=World2())
    with pytest.raises(NotImplementedError):
        m.build()

    m = model_for(g, ops)
    assert m.user_cholesky_factor is None and m.method == 'HybridSVD'
    m.precompute_auxiliary_matrix = True                     # accepted; same model
    m.build(return_factors=True)
    assert m.factors['userid'].shape == (int(g['train_shape'][0]), int(g['rank']))
    W = m.factors['itemid']
    F = m.item_cholesky_factor
    vl, vr = m.get_item_projector()
    assert np.allclose(F.dot(W), vr, atol=1e-12) and np.allclose(F.T.solve(W), vl, atol=1e-10)
    K = ref.relations(g).toarray() + np.eye(W.shape[0])
    Lp = F.L
    R = np.zeros_like(Lp)
    R[:] = Lp[np.ix_(F.perm, F.perm)]                        # R = P^T L P in external ids
    assert np.allclose(R @ R.T, K, atol=1e-12)
    old = m.item_cholesky_factor
    m.features_weight = 0.9                                  # re-factored at once, model renewed
    assert m.item_cholesky_factor is not old and not m._is_ready
    assert np.isclose(m.item_cholesky_factor.beta, 1 / 9)
