"""The Gram-image op of the item-weight models (HipOps._gram_image behind i2i_build, ease_gram and slim_gram): the three
layouts built from one device CSR hold the same A^T A, each with its own diagonal, rows and leading dimension.

Feedback is integer-valued in 1..5 over 40 users, so every sum is an integer far below 2^24: exact in fp64 (and in the
certified fp32 image of i2i_build), no tolerance anywhere.  The sizes: a multiple of 8 and of 64, one below a tile, and 70,
where the two leading dimensions differ (72 and 128)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_USERS = 40
LAM = 2.5


@pytest.mark.parametrize('n_items', [8, 63, 64, 70])
def test_three_layouts_of_one_gram_matrix(n_items, hip_ops):
    from polara_amd import ease, i2i, slim
    rng = np.random.default_rng(900 + n_items)
    X = np.where(rng.random((N_USERS, n_items)) < 0.3, rng.integers(1, 6, (N_USERS, n_items)), 0).astype(np.float64)
    empty = n_items // 2
    X[:, empty] = 0                                             # an item column with no entries
    X[0, 0] = 3.0                                               # and one that surely has some
    u, i = np.nonzero(X)
    A = hip_ops.csr_from_coo(u, i, X[u, i], X.shape)
    G = X.T @ X
    squares = np.diag(G).copy()
    off = G - np.diag(squares)
    assert off.any() and squares[empty] == 0 and not off[empty].any()

    C, dtype = hip_ops.i2i_build(A)
    K = hip_ops.to_host(hip_ops.ease_gram(A, LAM))
    S = hip_ops.to_host(hip_ops.slim_gram(A))
    C = C.double().cpu().numpy()                                # the certified fp32 image widens exactly
    ld, ld_chol = i2i.leading_dim(n_items), ease.chol_leading_dim(n_items)
    assert dtype == 'float32' and ld == slim.gram_leading_dim(n_items) == -(-n_items // 8) * 8
    assert C.shape == S.shape == (n_items, ld) and K.shape == (ld_chol, ld_chol) and ld_chol == -(-n_items // 64) * 64
    assert n_items != 70 or (ld, ld_chol) == (72, 128)

    n = n_items
    for name, image, diagonal in (('i2i', C, np.zeros(n)), ('cholesky', K[:n], squares + LAM), ('slim', S, squares)):
        block = image[:, :n]
        assert np.array_equal(np.diag(block), diagonal), name
        assert np.array_equal(block - np.diag(np.diag(block)), off), name
    assert not C[:, n:].any() and not S[:, n:].any()            # the pad columns their docstrings promise
