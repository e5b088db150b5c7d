"""EASE, host side (no GPU): the NumPy restatement (tests/ease_reference.py) against the optimality conditions of its own
definition, the planning and the memory guard of the device path (polara_amd/ease.py) against the library's pk_* planning
functions, and the stated limits of the model."""
import numpy as np
import pytest

import ease_reference as ref


@pytest.mark.parametrize('name', sorted(ref.FIXTURES))
@pytest.mark.parametrize('lam', ref.LAMBDAS)
@pytest.mark.parametrize('implicit', [False, True])
def test_restatement_satisfies_its_optimality_conditions(name, lam, implicit):
    """Stationarity of |X - X B|^2 + lam |B|^2 under diag(B) = 0: (G + lam I) B - G vanishes off the diagonal (on the
    diagonal sits the multiplier of the constraint)."""
    idx, val, shape = ref.training(name)
    A = ref.training_matrix(idx, val, shape, implicit)
    B, P = ref.ease_weights(A, lam)
    assert not np.diag(B).any()
    G = ref.gram(A, 0.0)
    R = (G + lam * np.eye(shape[1])) @ B - G
    off = R - np.diag(np.diag(R))
    assert np.abs(off).max() <= 1e-10 * np.abs(G).max()
    # B and d carry all of P (a division and a product per entry: two roundings)
    assert np.abs(ref.precision_from_weights(B, np.diag(P)) - P).max() <= 4 * 2.0 ** -53 * np.abs(P).max()
    T = ref.training_matrix(idx[:50], val[:50], shape, implicit)
    S = ref.ease_scores(B, T)
    assert S.shape == shape and np.allclose(S, T.toarray() @ B, rtol=1e-12, atol=1e-12)


def test_fixtures_cover_the_cases():
    for name, (n_users, n_items, per) in ref.FIXTURES.items():
        idx, val, shape = ref.training(name)
        assert shape == (n_users, n_items) and len(np.unique(idx[:, 1])) == n_items
        assert 0.8 * per <= len(val) / n_users <= 1.25 * per
        assert np.array_equal(val, np.round(val))
        _, half, _ = ref.training(name, half_steps=True)
        assert np.array_equal(2 * half, np.round(2 * half)) and not np.array_equal(half, np.round(half))
        (tu, ti, tv), hold, tshape = ref.test_rows(name)
        rows = set(tu.tolist())
        assert rows == set(range(len(hold[0]) - 3)) and (np.diff(tu) >= 0).all()          # the last three rows are empty
        assert not tv[tu == 1].any() and not tv[tu == 8].any() and (tu == 2).sum() == int(0.6 * n_items)
        assert tshape == (len(hold[0]), n_items)


def test_planning_matches_the_library():
    from polara_amd import _lib, ease
    lib = _lib.load()
    for n in (1, 15, 16, 17, 63, 64, 65, 129, 200, 1000, 2048, 2049, 2113, 4099, 26744, 100000):
        assert ease.chol_leading_dim(n) == lib.pk_hybrid_ld(n)
        assert ease.weights_leading_dim(n) == lib.pk_i2i_ld(n)
        assert ease.trtri_work_bytes(n) == lib.pk_trtri_work_bytes(n)
        assert ease.chol_image_bytes(n) == lib.pk_hybrid_ld(n) ** 2 * 8
        assert ease.weights_image_bytes(n) == n * lib.pk_i2i_ld(n) * 8
    assert ease.trtri_work_bytes(64) == 0 and ease.trtri_work_bytes(65) == 64 * 64 * 8
    assert ease.trtri_work_bytes(0) == lib.pk_trtri_work_bytes(0) == 0
    # ML-20M shape: 418 tile rows, the longest panel has 417 tiles in 14 chunks
    assert ease.trtri_work_bytes(26744) == 14 * 417 * 64 * 64 * 8
    assert ease.MAX_TOPK == lib.pk_i2i_max_topk() == 1024


def test_memory_guard():
    from polara_amd import ease
    n = 26744
    need = 26752 * 26752 * 8 + 26744 * 26744 * 8
    assert ease.check_build_memory(n, 2 * need) == need
    with pytest.raises(MemoryError, match=str(need)):
        ease.check_build_memory(n, 2 * need - 16)
    with pytest.raises(MemoryError, match=r'11\.45 GB'):
        ease.check_build_memory(n, 1e9)
    assert ease.check_build_memory(1, 2 * (64 * 64 * 8 + 8 * 8)) == 64 * 64 * 8 + 8 * 8       # one tile and one padded row


def _tiny_data():
    from polara_amd.data import ArrayData
    u, i, v = np.array([0, 0, 1]), np.array([0, 1, 1]), np.array([1.0, 2.0, 3.0])
    return ArrayData((u, i, v), n_users=2, n_items=2)


def test_model_attributes_and_export():
    import polara_amd
    from polara_amd.ease import EASEModel
    from polara_amd.models import RecommenderModel
    assert polara_amd.EASEModel is EASEModel and 'EASEModel' in polara_amd.__all__
    assert issubclass(EASEModel, RecommenderModel)
    m = EASEModel(_tiny_data())
    assert (m.method, m.regularization, m.implicit, m.dense_output, m._topk_limit) == ('EASE', 500.0, False, True, 1024)
    assert m._item_rank is None and m.item_weights is None and m.precision_diagonal is None


def test_bad_regularization_raises():
    from polara_amd.ease import EASEModel
    m = EASEModel(_tiny_data())
    for bad in (-1.0, -1e-300, float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='regularization'):
            m.regularization = bad
    assert m.regularization == 500.0
    m.regularization = 0                                       # allowed: it fails only where the matrix is singular
    assert m.regularization == 0.0


def test_settings_renew_the_model():
    from polara_amd.ease import EASEModel
    m = EASEModel(_tiny_data())
    m._is_ready, m._weights = True, object()
    m.regularization = 500.0                                   # unchanged: nothing happens
    m.implicit = False
    assert m._is_ready and m._weights is not None
    m.regularization = 10
    assert not m._is_ready and m._weights is None
    m._is_ready, m._weights = True, object()
    m.implicit = True
    assert not m._is_ready and m._weights is None


def test_sparse_branch_is_not_offered():
    from polara_amd.ease import EASEModel
    m = EASEModel(_tiny_data())
    m.dense_output = True
    with pytest.raises(NotImplementedError, match='dense'):
        m.dense_output = False
    assert m.dense_output is True


def test_multi_process_raises():
    from polara_amd.ease import EASEModel

    class TwoRanks:
        world, rank = 2, 0
    with pytest.raises(NotImplementedError):
        EASEModel(_tiny_data(), comm=TwoRanks()).build()


def test_topk_above_the_limit_raises():
    from polara_amd import ease, i2i
    assert i2i.check_topk(1024, 5000, ease.EASEModel._topk_limit) == 1024
    with pytest.raises(ValueError, match='1024'):
        i2i.check_topk(1025, 5000, ease.EASEModel._topk_limit)
