"""iALS++ on the device: the block-step kernel and the prediction kernel (csrc/ialspp.hip) against the NumPy restatement
(tests/ialspp_reference.py) within per-row and per-entry error bounds, the three properties of the step (one block = the exact
half-step, the exact solution is a fixed point, the objective never rises), per-row regularisation, determinism, refusals, and
the model — standard scenario, warm start, identical builds — against the restatement's fit.

The step bound (ialspp_reference.step_bounds), per row with eps = 2^-53, n entries, dw the block's width:
    |x^_pi - x_pi|_2 <= 4 kappa_2(H) eps [ (n + 2) S_H / |H|_2 + dw (3 dw + 1) + (n + 2) S_g / |g|_2 ] (|x0_pi|_2 + |x_pi|_2)
and per stored entry |e^ - e| <= n d eps (|e0| + sum_j |y_ij| |delta_j|).  The restatement is given the device's own G, R and
starting predictions, so that only the step is under test; every step test also asserts ON THE CPU that a step with the last
interaction of each row dropped lies at least `DROPPED_MARGIN` times outside the bound (measured: tests/test_ialspp_host.py).

Measured on the MI355X (every test prints its ratio): the largest error / bound of a block step is 0.043 for the rows (rank 17,
the one-column block) and 0.37 for the predictions (3 000 x 16 at rank 5); predictions 0.57 of their bound at rank 5 and 1e-3 at
rank 2048; one block against the exact half-step 7.2e-4 of the two bounds; the models' factors at 0.86 .. 0.99 d of 16 d."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import ials_reference as ials_ref
import ialspp_reference as ref
from ialspp_reference import DROPPED_MARGIN, STEP_CASES, start
from sweep_helpers import padding_is_zero, strided

pytestmark = pytest.mark.gpu


def device_csr(ops, C):
    return ops.csr(C.indptr, C.indices, np.asarray(C.data, dtype=np.float64), C.shape)


@functools.lru_cache(maxsize=None)
def device_matrix(ops, kind):
    return device_csr(ops, ials_ref.confidence_matrix(kind))


def check_block_step(ops, kind, rank, d, p0, lam, pad=0, lam_rows=None):
    """one block step on the device against the restatement on the device's own G, R and E; returns the largest error / bound
    of the rows and of the entries"""
    C = ials_ref.confidence_matrix(kind)
    Y = ials_ref.item_block(C.shape[1], rank)
    X0 = start(C, rank)
    Cd = device_matrix(ops, kind)
    Yd = strided(ops, Y, pad, 1) if pad else ops.to_device(Y)
    Xd = strided(ops, X0, pad, 0) if pad else ops.to_device(X0)
    Gd = ops.gram(Yd)
    G = ops.to_host(Gd)
    if pad:
        Gd = strided(ops, G, pad + 2, 2)
    p1 = min(p0 + d, rank)
    Rd = ops.tsmm(Xd, Gd[:, p0:p1])
    R = ops.to_host(Rd)
    if pad:
        Rd = strided(ops, R, pad + 1, 1)
    Ed = ops.ialspp_predict(Cd, Xd, Yd)
    E0 = ops.to_host(Ed).copy()
    reg = lam if lam_rows is None else ops.to_device(lam_rows)
    assert ops.ialspp_block_step(Cd, Yd, Xd, Ed, Gd, p0, d, reg, R=Rd) is Xd
    if pad:
        assert Yd.stride(0) > rank and Gd.stride(0) > rank and Xd.stride(0) > rank and Rd.stride(0) > p1 - p0
        assert padding_is_zero(Xd) and padding_is_zero(Rd)               # nothing written beside the rows
    got, gotE = ops.to_host(Xd), ops.to_host(Ed)
    lam_ref = lam if lam_rows is None else lam_rows
    want, wantE = X0.copy(), E0.copy()
    ref.block_step(C, Y, want, wantE, G, p0, d, lam_ref, R=R)
    rows, entries = ref.step_bounds(C, Y, G, lam_ref, X0, E0, p0, d, want, R=R)
    assert ref.dropped_interaction_margin(C, Y, G, lam_ref, X0, E0, p0, d, want, rows, R=R) >= DROPPED_MARGIN
    outside = np.r_[0:p0, p1:rank]
    assert np.array_equal(got[:, outside], X0[:, outside])              # the other columns keep their bits
    empty = np.diff(C.indptr) == 0
    assert empty.any() and not got[empty, p0:p1].any() and (rows[empty] == 0).all()           # exactly zero
    err, errE = np.linalg.norm(got - want, axis=1), np.abs(gotE - wantE)
    ratio, ratioE = (err[~empty] / rows[~empty]).max(), (errE[entries > 0] / entries[entries > 0]).max()
    print('block step %s rank %d d %d p0 %d lambda %g: largest error / bound = %.3g (rows), %.3g (predictions)'
          % (kind, rank, d, p0, lam, ratio, ratioE))
    assert (err <= rows).all(), ratio
    assert (errE <= entries).all(), ratioE
    return ratio, ratioE


@pytest.mark.parametrize('lam', [0.01, 1e-6])
@pytest.mark.parametrize('rank, d, p0', STEP_CASES)
def test_block_step_matches_the_restatement(hip_ops, rank, d, p0, lam):
    """40 rows x 1 100 columns, row lengths 0 .. 9, 31 .. 33, 63 .. 65 around the staging chunk, 257 and 1 000 (several chunks);
    every block width, full, padded and a single column, first and last block"""
    check_block_step(hip_ops, 'wide', rank, d, p0, lam)


def test_block_step_honours_leading_dimensions(hip_ops):
    check_block_step(hip_ops, 'wide', 100, 64, 64, 0.01, pad=3)


def test_block_step_with_more_rows_than_one_wave_of_workgroups(hip_ops):
    check_block_step(hip_ops, 'tall', 5, 16, 0, 0.01)


def test_block_step_where_lambda_carries_a_singular_gram(hip_ops):
    assert np.linalg.matrix_rank(ials_ref.item_block(12, 16)) == 12
    check_block_step(hip_ops, 'narrow', 16, 16, 0, 0.01)


@pytest.mark.parametrize('rank', [1, 5, 64, 128, 129, 272, 512, 513, 2048])
def test_predictions_match_the_restatement(hip_ops, rank):
    """every instance of the kernel (2, 8, 32 columns per lane) at its ends, with leading dimensions; an entry is a sum of
    `rank` products: |e^ - e| <= rank eps sum |x_j| |y_j|"""
    ops = hip_ops
    C = ials_ref.confidence_matrix('wide')
    Y, X = ials_ref.item_block(C.shape[1], rank), start(C, rank)
    Ed = ops.ialspp_predict(device_matrix(ops, 'wide'), strided(ops, X), strided(ops, Y, 5, 2))
    rows = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr))
    bound = rank * ials_ref.EPS * np.einsum('ij,ij->i', np.abs(X[rows]), np.abs(Y[C.indices]))
    err = np.abs(ops.to_host(Ed) - ref.predict(C, X, Y))
    print('predict rank %d: largest error / bound = %.3g' % (rank, (err / bound).max()))
    assert Ed.shape == (C.nnz,) and (err <= bound).all()
    out = ops.empty(C.nnz)
    assert ops.ialspp_predict(device_matrix(ops, 'wide'), ops.to_device(X), ops.to_device(Y), out=out) is out
    assert ops.to_host(out).tobytes() == ops.to_host(Ed).tobytes()        # the leading dimensions change no bit


@pytest.mark.parametrize('rank, d', [(16, 16), (50, 64), (64, 64)])
def test_one_block_over_the_rank_is_the_exact_half_step(hip_ops, rank, d):
    ops = hip_ops
    C = ials_ref.confidence_matrix('wide')
    Y, X0 = ials_ref.item_block(C.shape[1], rank), start(C, rank)
    Cd, Yd, Xd = device_matrix(ops, 'wide'), ops.to_device(Y), ops.to_device(X0)
    Gd = ops.gram(Yd)
    G = ops.to_host(Gd)
    exact = ops.to_host(ops.ials_half_step(Cd, Yd, 0.01, G=Gd))
    E0 = ops.to_host(ops.ialspp_predict(Cd, Xd, Yd)).copy()
    ops.ialspp_half_sweep(Cd, Yd, Xd, Gd, 0.01, d)
    got = ops.to_host(Xd)
    want = ials_ref.half_step(C, Y, G, 0.01)
    bounds = ials_ref.row_bounds(C, Y, G, 0.01, want) + ref.step_bounds(C, Y, G, 0.01, X0, E0, 0, d, want)[0]
    err = np.linalg.norm(got - exact, axis=1)
    full = bounds > 0
    print('one block, rank %d: largest distance to the exact half-step / (row bound + step bound) = %.3g' % (rank, (err[full] / bounds[full]).max()))
    assert (err <= bounds).all() and not got[~full].any()


def test_the_exact_solution_is_a_fixed_point(hip_ops):
    ops = hip_ops
    C = ials_ref.confidence_matrix('wide')
    rank, d = 50, 16
    Y = ials_ref.item_block(C.shape[1], rank)
    Cd, Yd = device_matrix(ops, 'wide'), ops.to_device(Y)
    Gd = ops.gram(Yd)
    G = ops.to_host(Gd)
    Xd = ops.ials_half_step(Cd, Yd, 0.01, G=Gd)
    Ed = ops.ialspp_predict(Cd, Xd, Yd)
    moved, allowed = np.zeros(C.shape[0]), np.zeros(C.shape[0])
    for p0 in range(0, rank, d):
        X0, E0 = ops.to_host(Xd).copy(), ops.to_host(Ed).copy()
        ops.ialspp_block_step(Cd, Yd, Xd, Ed, Gd, p0, d, 0.01)
        X1 = ops.to_host(Xd)
        moved += np.linalg.norm(X1 - X0, axis=1)
        allowed += ref.step_bounds(C, Y, G, 0.01, X0, E0, p0, d, X1)[0]
    full = allowed > 0
    print('fixed point: largest move / bound = %.3g, largest move %.3g' % ((moved[full] / allowed[full]).max(), moved.max()))
    assert (moved <= allowed).all() and moved.max() <= 1e-12 * np.linalg.norm(X1, axis=1).max()


@pytest.mark.parametrize('d', [16, 32, 64])
def test_predictions_after_a_half_sweep_are_those_of_the_result(hip_ops, d):
    ops = hip_ops
    rank = 100
    C = ials_ref.confidence_matrix('wide')
    Y, X0 = ials_ref.item_block(C.shape[1], rank), start(C, rank)
    Cd, Yd, Xd = device_matrix(ops, 'wide'), ops.to_device(Y), ops.to_device(X0)
    _, Ed = ops.ialspp_half_sweep(Cd, Yd, Xd, ops.gram(Yd), 0.01, d)
    again = ops.to_host(ops.ialspp_predict(Cd, Xd, Yd))
    X1 = ops.to_host(Xd)
    n = np.repeat(np.diff(C.indptr), np.diff(C.indptr))
    rows = np.repeat(np.arange(C.shape[0]), np.diff(C.indptr))
    # the entry bound of a block step, n d eps (|e| + sum_j |y_j| |delta_j|), with |e| <= S = sum_j |y_j| (|x0_j| + |x1_j|) over
    # all columns in every block and the deltas of all blocks together <= S: (blocks + 1) n d eps S; the prediction of the
    # result is itself a sum of `rank` products: rank eps S
    blocks = -(-rank // d)
    S = (np.abs(Y[C.indices]) * (np.abs(X0[rows]) + np.abs(X1[rows]))).sum(axis=1)
    bound = ((blocks + 1) * n * d + rank) * ials_ref.EPS * S
    err = np.abs(ops.to_host(Ed) - again)
    print('half-sweep d %d: largest drift of the predictions / bound = %.3g (%.3g absolute)' % (d, (err / bound).max(), err.max()))
    assert (err <= bound).all()


def test_the_objective_never_rises(hip_ops):
    ops = hip_ops
    rank, d = 100, 32
    C = ials_ref.confidence_matrix('wide')
    Ct = sps.csr_matrix(C.T)
    Ct.sort_indices()
    Cd = device_matrix(ops, 'wide')
    Y, X = ials_ref.item_block(C.shape[1], rank), start(C, rank)
    Yd, Xd = ops.to_device(Y), ops.to_device(X)
    values = [ref.objective_terms(C, X, Y, 0.01, 0.01)]
    for M, A, B in ((Cd, Xd, Yd), (Cd.T, Yd, Xd)):                      # a user half-sweep, then an item half-sweep
        G = ops.gram(B)
        E = ops.ialspp_predict(M, A, B)
        for p0 in range(0, rank, d):
            ops.ialspp_block_step(M, B, A, E, G, p0, d, 0.01)
            values.append(ref.objective_terms(C, ops.to_host(Xd), ops.to_host(Yd), 0.01, 0.01))
    assert np.array_equal(ops.to_host(Cd.T.indices), Ct.indices)
    f = np.array([v[0] for v in values])
    slack = np.array([v[2] * ials_ref.EPS * v[1] for v in values])
    print('objective over two half-sweeps: %s; largest rise / slack = %.3g' % (f, ((f[1:] - f[:-1]) / slack[:-1]).max()))
    assert len(f) == 9 and (f[1:] - f[:-1] <= slack[:-1]).all() and f[-1] < 0.5 * f[0]


def test_per_row_regularization(hip_ops):
    ops = hip_ops
    C = ials_ref.confidence_matrix('wide')
    rank, d = 33, 32
    Y, X0 = ials_ref.item_block(C.shape[1], rank), start(C, rank)
    Cd, Yd = device_matrix(ops, 'wide'), ops.to_device(Y)
    Gd = ops.gram(Yd)
    runs = []
    for reg in (0.01, ops.to_device(np.full(C.shape[0], 0.01))):         # a vector of equal values: the bits of the scalar path
        Xd = ops.to_device(X0)
        _, Ed = ops.ialspp_half_sweep(Cd, Yd, Xd, Gd, reg, d)
        runs.append((ops.to_host(Xd), ops.to_host(Ed)))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    lam_rows = ref.row_regularization(C, 0.01, 1.0, 1.0)                 # exponent 1: lambda from 11.0 to 21.0
    assert lam_rows.min() == 11.0 and lam_rows.max() == 21.0
    for p0 in (0, 32):
        check_block_step(ops, 'wide', rank, d, p0, 0.01, lam_rows=lam_rows)
    with pytest.raises(ValueError, match='per-row regularization'):
        ops.ialspp_half_sweep(Cd, Yd, ops.to_device(X0), Gd, ops.to_device(np.full(C.shape[0] + 1, 0.01)), d)
    got = ops.ialspp_loss(Cd, ops.to_device(X0), Yd, ops.to_device(lam_rows), 0.5)
    want = ref.objective(C, X0, Y, lam_rows, 0.5)
    assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize('rank', [50, 272])
def test_loss_matches_the_dense_objective(hip_ops, rank):
    """up to rank 128 the sparse term is the iALS kernel's, above it is summed from the predictions"""
    ops = hip_ops
    C = ials_ref.confidence_matrix('wide')
    Y, X = ials_ref.item_block(C.shape[1], rank), ials_ref.item_block(C.shape[0], rank, seed=1)
    got = ops.ialspp_loss(device_matrix(ops, 'wide'), strided(ops, X), strided(ops, Y, 5, 2), 0.01, 0.01)
    want = ref.objective(C, X, Y, 0.01, 0.01)
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)


def test_block_step_is_deterministic_and_independent_of_the_row_order(hip_ops):
    ops = hip_ops
    for kind, rank, d in (('wide', 100, 64), ('wide', 50, 16), ('tall', 5, 16)):
        Cd = device_matrix(ops, kind)
        Yd = ops.to_device(ials_ref.item_block(Cd.shape[1], rank))
        G = ops.gram(Yd)
        X0 = start(Cd, rank)
        order = ops._ials_row_order(Cd)
        runs = []
        for row_order in (None, None, torch.flip(order, [0]).contiguous()):
            Xd = ops.to_device(X0)
            Ed = ops.ialspp_predict(Cd, Xd, Yd)
            for p0 in range(0, rank, d):
                ops.ialspp_block_step(Cd, Yd, Xd, Ed, G, p0, d, 0.01, row_order=row_order)
            runs.append(ops.to_host(Xd).tobytes() + ops.to_host(Ed).tobytes())
        assert runs[0] == runs[1] == runs[2]


def test_not_positive_definite_rows_are_counted_and_left_alone(hip_ops):
    """lambda = 0, rank 16, 12 columns, columns 12 .. 15 of Y zeros: the trailing 4 x 4 block of every H is exactly zero and
    pivot 12 is exactly 0 in any order of summation: every non-empty row is refused, no empty one, X and E keep their bits."""
    ops = hip_ops
    C = ials_ref.confidence_matrix('narrow')
    Y = ials_ref.item_block(12, 16)
    Y[:, 12:] = 0.0
    X0 = start(C, 16)
    Cd, Yd, Xd = device_matrix(ops, 'narrow'), ops.to_device(Y), ops.to_device(X0)
    Ed = ops.ialspp_predict(Cd, Xd, Yd)
    E0 = ops.to_host(Ed).copy()
    nonempty = np.flatnonzero(np.diff(C.indptr))
    assert nonempty[0] > 0
    with pytest.raises(ValueError, match=r'%d row\(s\).*first is row %d\b' % (len(nonempty), nonempty[0])):
        ops.ialspp_block_step(Cd, Yd, Xd, Ed, ops.gram(Yd), 0, 16, 0.0)
    got = ops.to_host(Xd)
    assert np.array_equal(got[nonempty], X0[nonempty]) and np.array_equal(ops.to_host(Ed), E0)
    # a block whose columns of Y are all zero, in a wider rank: H = 0 exactly
    Y = ials_ref.item_block(12, 40)
    Y[:, 32:] = 0.0
    X0 = start(C, 40)
    Yd, Xd = ops.to_device(Y), ops.to_device(X0)
    Ed = ops.ialspp_predict(Cd, Xd, Yd)
    E0 = ops.to_host(Ed).copy()
    with pytest.raises(ValueError, match=r'%d row\(s\).*first is row %d\b' % (len(nonempty), nonempty[0])):
        ops.ialspp_block_step(Cd, Yd, Xd, Ed, ops.gram(Yd), 32, 32, 0.0)
    assert np.array_equal(ops.to_host(Xd)[nonempty], X0[nonempty]) and np.array_equal(ops.to_host(Ed), E0)
    # a NaN pivot counts too: one confidence of row 5 is NaN, lambda carries the other rows
    data = np.array(C.data)
    assert C.indptr[6] > C.indptr[5]
    data[C.indptr[5]] = np.nan
    Cn = ops.csr(C.indptr, C.indices, data, C.shape)
    Y = ials_ref.item_block(12, 16)
    X0 = start(C, 16)
    Yd, Xd = ops.to_device(Y), ops.to_device(X0)
    Ed = ops.ialspp_predict(Cn, Xd, Yd)
    with pytest.raises(ValueError, match=r'1 row\(s\).*first is row 5\b'):
        ops.ialspp_block_step(Cn, Yd, Xd, Ed, ops.gram(Yd), 0, 16, 0.01)
    good = ops.to_device(X0)
    ops.ialspp_half_sweep(device_matrix(ops, 'narrow'), Yd, good, ops.gram(Yd), 0.01, 16)
    got, rest = ops.to_host(Xd), np.arange(C.shape[0]) != 5
    assert np.array_equal(got[5], X0[5]) and np.array_equal(got[rest], ops.to_host(good)[rest])


def test_column_ids_outside_the_matrix_contribute_nothing(hip_ops):
    ops = hip_ops
    C = ials_ref.confidence_matrix('narrow')
    rank = 16
    Y, X0 = ials_ref.item_block(12, rank), start(C, rank)
    indices = C.indices.copy()
    moved = C.indices >= 10                                              # columns 10 and 11 fall outside a matrix of 10 columns
    kept = sps.csr_matrix((C.data[~moved], C.indices[~moved], np.concatenate(([0], np.cumsum(~moved)))[C.indptr]), shape=(30, 10))
    indices[moved] = np.where(C.indices[moved] == 10, -1, 10)
    Cbad = ops.csr(C.indptr, indices, C.data, (30, 10))
    Ckept = device_csr(ops, kept)
    Yd = ops.to_device(Y[:10])
    G = ops.gram(Yd)
    Xa, Xb = ops.to_device(X0), ops.to_device(X0)
    _, Ea = ops.ialspp_half_sweep(Cbad, Yd, Xa, G, 0.01, 16)
    _, Eb = ops.ialspp_half_sweep(Ckept, Yd, Xb, G, 0.01, 16)
    Ea, Eb = ops.to_host(Ea), ops.to_host(Eb)
    assert not Ea[moved].any() and np.allclose(Ea[~moved], Eb, rtol=0, atol=1e-13)
    assert np.allclose(ops.to_host(Xa), ops.to_host(Xb), rtol=0, atol=1e-13)


def test_block_step_checks_its_arguments(hip_ops):
    ops = hip_ops
    Cd = device_matrix(ops, 'narrow')
    top = ops.ialspp_max_rank()
    assert top == ref.MAX_RANK == 2048 and ops.ialspp_block_sizes() == ref.BLOCK_SIZES == (16, 32, 64)
    nnz = int(Cd.indices.numel())
    X, Y, E, G = ops.zeros(30, 20), ops.zeros(12, 20), ops.zeros(nnz), ops.zeros(20, 20)
    with pytest.raises(ValueError, match='rank %d' % (top + 1)):
        ops.ialspp_predict(Cd, ops.zeros(30, top + 1), ops.zeros(12, top + 1))
    with pytest.raises(ValueError, match='block of shape'):
        ops.ialspp_block_step(Cd, ops.zeros(11, 20), X, E, G, 0, 16, 0.01)
    with pytest.raises(ValueError, match='block of shape'):
        ops.ialspp_block_step(Cd, Y, ops.zeros(29, 20), E, G, 0, 16, 0.01)
    with pytest.raises(ValueError, match='predictions of shape'):
        ops.ialspp_block_step(Cd, Y, X, ops.zeros(nnz + 1), G, 0, 16, 0.01)
    with pytest.raises(ValueError, match='block size 24'):
        ops.ialspp_block_step(Cd, Y, X, E, G, 0, 24, 0.01)
    with pytest.raises(ValueError, match='block start 20'):
        ops.ialspp_block_step(Cd, Y, X, E, G, 20, 16, 0.01)
    with pytest.raises(ValueError, match='G of shape'):
        ops.ialspp_block_step(Cd, Y, X, E, ops.zeros(20, 19), 0, 16, 0.01)
    with pytest.raises(ValueError, match='R of shape'):
        ops.ialspp_block_step(Cd, Y, X, E, G, 16, 16, 0.01, R=ops.zeros(30, 16))
    with pytest.raises(ValueError, match='row_order'):
        ops.ialspp_block_step(Cd, Y, X, E, G, 0, 16, 0.01, row_order=torch.arange(30, device=ops.device))


# ---- the model -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built_model(ops, name):
    m = ref.model_for(ref.model_case(name), ops, compute_loss=True)
    m.build()
    return m


@pytest.mark.parametrize('name', list(ref.MODEL_CASES))
def test_model_matches_the_restated_fit(hip_ops, name):
    """rank 272 is above the fused serving rank: its lists come from the exact-rows path"""
    case = ref.model_case(name)
    m = built_model(hip_ops, name)
    X, Y = m.factors['userid'], m.factors['itemid']
    assert m.method == 'iALS++' and X.shape == case['X'].shape and Y.shape == case['Y'].shape and X.dtype == Y.dtype == np.float64
    dist = max(ials_ref.rel_distance(X, case['X']), ials_ref.rel_distance(Y, case['Y']))
    print('model %s: d = %.3g, device distance = %.3g (%.2f d)' % (name, case['d'], dist, dist / case['d']))
    assert 0 < case['d'] < 1e-11
    assert dist <= 16 * case['d'], (dist, case['d'])
    assert np.array_equal(m._get_test_data()[2], case['test_users'])
    recs = m.get_recommendations()
    assert recs.dtype == np.int64 and (case['gaps'] >= ref.MIN_GAP).all()
    ials_ref.check_lists(recs, case['lists'], case['gaps'], min_gap=0.0, max_left_out=0.0)      # every row
    loss = np.array(m.loss_history)
    assert len(loss) == 2 * case['epochs'] == len(case['loss']) and len(m.iterations_time) == case['epochs']
    assert (loss[1:] <= loss[:-1] * (1 + 1e-12)).all()
    assert np.allclose(loss, case['loss'], rtol=1e-9, atol=0)
    s, _ = m.slice_recommendations(*m._get_test_data()[:2], 0, 5, m._get_test_data()[2])
    assert np.allclose(s, case['X'][case['test_users'][:5]] @ case['Y'].T, rtol=0, atol=1e-10)


def test_warm_start_runs_the_fold_in_sweeps(hip_ops):
    ops = hip_ops
    w = ref.warm_case('r16')
    case = w['case']
    m = ref.model_for(case, ops, data=ials_ref.warm_data(w))
    m.build()
    assert ials_ref.rel_distance(m.factors['itemid'], case['Y']) <= 16 * case['d']
    tu, ti, tf = w['test']
    keep = tf != 1.0
    Cw = sps.csr_matrix((np.log2(tf[keep]), (tu[keep], ti[keep])), shape=(w['n_new'], case['n_items']))
    Cw.sort_indices()
    Yd, Gd = m._item_factors_block()
    Y, G = ops.to_host(Yd), ops.to_host(Gd)
    # rank 16 in one block: every sweep lands on the exact fold-in, which is ImplicitALS's
    got = ops.to_host(m.fold_in())
    want = ref.fold_in(Cw, Y, G, ref.LAMBDA, 16, m.fold_in_sweeps)
    exact = ials_ref.half_step(Cw, Y, G, ref.LAMBDA)
    bounds = ials_ref.row_bounds(Cw, Y, G, ref.LAMBDA, exact)
    plain = ials_ref.model_for(case, ops, data=ials_ref.warm_data(w))
    plain.factors, plain._is_ready = dict(m.factors), True
    als = ops.to_host(plain.fold_in())
    folded = bounds > 0
    assert folded.sum() >= w['n_new'] - 3 and not got[~folded].any()
    for other, what in ((want, 'the restatement'), (als, 'ImplicitALS.fold_in')):
        err = np.linalg.norm(got - other, axis=1)
        print('warm start against %s: largest error / (2 x row bound) = %.3g' % (what, (err[folded] / (2 * bounds[folded])).max()))
        assert (err <= 2 * bounds).all()                                 # both sides carry the half-step's error
    recs = m.get_recommendations()
    lists, gaps = ials_ref.lists_and_gaps(exact @ Y.T, (tu, ti))
    ials_ref.check_lists(recs, lists, gaps)
    # several blocks: eight sweeps of d = 16 at rank 40 against the restatement's eight
    case = ref.model_case('r40')
    m = built_model(ops, 'r40')
    rng = np.random.RandomState(5)
    rows = np.repeat(np.arange(20), 6)
    cols = np.concatenate([np.sort(rng.permutation(case['n_items'])[:6]) for _ in range(20)])
    Cw = sps.csr_matrix((rng.randint(2, 6, size=120).astype(np.float64), (rows, cols)), shape=(20, case['n_items']))
    Yd, Gd = m._item_factors_block()
    Y, G = ops.to_host(Yd), ops.to_host(Gd)
    Xd = ops.zeros(20, 40)
    for _ in range(m.fold_in_sweeps):
        ops.ialspp_half_sweep(device_csr(ops, Cw), Yd, Xd, Gd, ref.LAMBDA, 16)
    want = ref.fold_in(Cw, Y, G, ref.LAMBDA, 16, m.fold_in_sweeps)
    d = ials_ref.rel_distance(ref.fold_in(Cw, Y, G, ref.LAMBDA, 16, m.fold_in_sweeps, solve=ials_ref.lapack_solve), want)
    dist = ials_ref.rel_distance(ops.to_host(Xd), want)
    print('eight sweeps at rank 40: d = %.3g, device distance %.3g' % (d, dist))
    assert dist <= 16 * d


def test_two_seeded_builds_give_identical_bits(hip_ops):
    case = ref.model_case('r40')
    first = built_model(hip_ops, 'r40')
    again = ref.model_for(case, hip_ops)
    again.build()
    assert again.factors['userid'].tobytes() == first.factors['userid'].tobytes()
    assert again.factors['itemid'].tobytes() == first.factors['itemid'].tobytes()
    assert np.array_equal(again.get_recommendations(), first.get_recommendations())
