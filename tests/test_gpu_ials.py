"""Implicit ALS on the device: the half-step kernel (csrc/ials.hip) against the NumPy restatement (tests/ials_reference.py) within
a per-row error bound, its determinism, its refusal of systems that are not positive definite, the loss kernel, and the model
— standard scenario, warm start, the scaled composition — against the restatement's fit.

The half-step bound (ials_reference.row_bounds), per row with eps = 2^-53, n entries, S_A = |G|_2 + lambda + sum |c - 1| |y_i|^2,
S_b = sum c |y_i|:
    |x^_u - x_u|_2 <= 4 kappa_2(A_u) eps [ (n + 2) S_A / |A_u|_2 + k (3 k + 1) + n S_b / |b_u|_2 ] |x_u|_2
and exactly 0 for an empty row.  The restatement is given the device's own G, so that only the new kernel is under test; every
test also asserts ON THE CPU that a result with one interaction dropped lies at least 6e7 times outside the bound."""
import functools

import numpy as np
import pytest
import torch

import ials_reference as ref
from polara_amd import ials
from polara_amd.models import ScaledMatrixMixin
from sweep_helpers import strided

pytestmark = pytest.mark.gpu

RANKS = [1, 3, 5, 15, 16, 17, 33, 50, 64, 65, 128]
DROPPED_MARGIN = 6e7


def device_csr(ops, C):
    return ops.csr(C.indptr, C.indices, np.asarray(C.data, dtype=np.float64), C.shape)


@functools.lru_cache(maxsize=None)
def device_matrix(ops, kind):
    return device_csr(ops, ref.confidence_matrix(kind))


def check_half_step(ops, kind, rank, lam, pad=0):
    """one half-step on the device against the restatement on the device's own G; returns the largest error / bound"""
    C = ref.confidence_matrix(kind)
    Y = ref.item_block(C.shape[1], rank)
    Cd = device_matrix(ops, kind)
    Yd = strided(ops, Y, pad, 1) if pad else ops.to_device(Y)
    Gd = ops.gram(Yd)
    G = ops.to_host(Gd)
    if pad:
        Gd = strided(ops, G, pad + 2, 2)
    out = strided(ops, np.full((C.shape[0], rank), np.nan), pad, 0) if pad else None
    Xd = ops.ials_half_step(Cd, Yd, lam, out=out, G=Gd)
    if pad:
        assert Xd is out and Yd.stride(0) > rank and Gd.stride(0) > rank and Xd.stride(0) > rank
        base = out._base.clone()
        assert not bool(base[:, rank:].any())                           # nothing written beside the rows
    got = ops.to_host(Xd)
    want = ref.half_step(C, Y, G, lam)
    bounds = ref.row_bounds(C, Y, G, lam, want)
    assert ref.dropped_interaction_margin(C, Y, G, lam, want, bounds) >= DROPPED_MARGIN      # the tolerance cannot hide a lost term
    err = np.linalg.norm(got - want, axis=1)
    empty = np.diff(C.indptr) == 0
    assert empty.any() and not got[empty].any() and (bounds[empty] == 0).all()               # exactly zero
    ratio = (err[~empty] / bounds[~empty]).max()
    print('half-step %s rank %d lambda %g: largest error / bound = %.3g' % (kind, rank, lam, ratio))
    assert (err <= bounds).all(), ratio
    return ratio


@pytest.mark.parametrize('lam', [0.01, 1e-6])
@pytest.mark.parametrize('rank', RANKS)
def test_half_step_matches_the_restatement(hip_ops, rank, lam):
    """40 rows x 1 100 columns, row lengths 0 .. 9 around the K = 4 groups, 31 .. 65 around the staging chunks, 257 and 1 000
    (several chunks); every rank at which the kernel takes another instance or pads differently"""
    check_half_step(hip_ops, 'wide', rank, lam)


def test_half_step_honours_leading_dimensions(hip_ops):
    check_half_step(hip_ops, 'wide', 17, 0.01, pad=3)


def test_half_step_with_more_rows_than_one_wave_of_workgroups(hip_ops):
    check_half_step(hip_ops, 'tall', 5, 0.01)


def test_half_step_where_lambda_carries_a_singular_gram(hip_ops):
    assert np.linalg.matrix_rank(ref.item_block(12, 16)) == 12
    check_half_step(hip_ops, 'narrow', 16, 0.01)


def test_half_step_is_deterministic_and_independent_of_the_row_order(hip_ops):
    ops = hip_ops
    for kind, rank in (('wide', 50), ('tall', 5)):
        Cd = device_matrix(ops, kind)
        Yd = ops.to_device(ref.item_block(Cd.shape[1], rank))
        G = ops.gram(Yd)
        first = ops.to_host(ops.ials_half_step(Cd, Yd, 0.01, G=G))
        again = ops.to_host(ops.ials_half_step(Cd, Yd, 0.01, G=G))
        order = ops._ials_row_order(Cd)
        lengths = np.diff(ops.to_host(Cd.indptr))[ops.to_host(order)]
        assert (np.diff(lengths) <= 0).all() and sorted(ops.to_host(order)) == list(range(Cd.shape[0]))      # longest rows first
        rev = ops.to_host(ops.ials_half_step(Cd, Yd, 0.01, G=G, row_order=torch.flip(order, [0]).contiguous()))
        assert first.tobytes() == again.tobytes() == rev.tobytes()


def test_not_positive_definite_rows_are_counted_and_zeroed(hip_ops):
    """lambda = 0, rank 16, 12 columns.  With random rows of Y the pivots that are zero in exact arithmetic come out as
    roundings of either sign; here columns 12 .. 15 of Y are zeros, so the trailing 4 x 4 block of every A_u is exactly zero and
    pivot 12 is exactly 0 in any order of summation: every non-empty row is refused, no empty one."""
    ops = hip_ops
    C = ref.confidence_matrix('narrow')
    Y = ref.item_block(12, 16)
    Y[:, 12:] = 0.0
    Cd, Yd = device_matrix(ops, 'narrow'), ops.to_device(Y)
    out = ops.to_device(np.full((C.shape[0], 16), 7.0))
    nonempty = np.flatnonzero(np.diff(C.indptr))
    assert nonempty[0] > 0
    with pytest.raises(ValueError, match=r'%d row\(s\).*first is row %d\b' % (len(nonempty), nonempty[0])):
        ops.ials_half_step(Cd, Yd, 0.0, out=out)
    assert not ops.to_host(out).any()
    with pytest.raises(ref.NotPositiveDefinite, match=r'%d row\(s\).*first is row %d\b' % (len(nonempty), nonempty[0])):
        ref.half_step(C, Y, Y.T @ Y, 0.0)
    # a NaN pivot counts too: one confidence of row 5 is NaN, lambda carries the other rows
    data = np.array(C.data)
    assert C.indptr[6] > C.indptr[5]
    data[C.indptr[5]] = np.nan
    Cn = ops.csr(C.indptr, C.indices, data, C.shape)
    Y = ref.item_block(12, 16)
    Yd = ops.to_device(Y)
    out = ops.to_device(np.full((C.shape[0], 16), 7.0))
    with pytest.raises(ValueError, match=r'1 row\(s\).*first is row 5\b'):
        ops.ials_half_step(Cn, Yd, 0.01, out=out)
    got = ops.to_host(out)
    good = ops.to_host(ops.ials_half_step(device_matrix(ops, 'narrow'), Yd, 0.01))
    rest = np.arange(C.shape[0]) != 5
    assert not got[5].any() and np.array_equal(got[rest], good[rest])


def test_half_step_checks_its_arguments(hip_ops):
    ops = hip_ops
    Cd = device_matrix(ops, 'narrow')
    top = ops.ials_max_rank()
    assert top == ref.MAX_RANK == 128
    with pytest.raises(ValueError, match='rank %d' % (top + 1)):
        ops.ials_half_step(Cd, ops.zeros(12, top + 1), 0.01)
    with pytest.raises(ValueError, match='block of shape'):
        ops.ials_half_step(Cd, ops.zeros(11, 4), 0.01)
    with pytest.raises(ValueError, match='block of shape'):
        ops.ials_half_step(Cd, ops.zeros(12, 4), 0.01, out=ops.zeros(29, 4))
    with pytest.raises(ValueError, match='row_order'):
        ops.ials_half_step(Cd, ops.zeros(12, 4), 0.01, row_order=torch.arange(30, device=ops.device))
    Y = ops.zeros(12, top + 1)
    rc = ops.lib.pk_ials_half_step_f64(ops.stream(), 30, 12, top + 1, Cd.indptr.data_ptr(), Cd.indices.data_ptr(), Cd.values.data_ptr(),
                                       None, Y.data_ptr(), top + 1, Y.data_ptr(), top + 1, 0.01, ops.zeros(30, top + 1).data_ptr(), top + 1,
                                       ops.zeros(2).data_ptr(), ops.zeros(64).data_ptr())
    assert rc == -1 and b'rank' in ops.lib.pk_last_error()              # PK_E_INVALID, nothing enqueued


def test_loss_kernel_matches_the_dense_objective(hip_ops):
    ops = hip_ops
    C = ref.confidence_matrix('wide')
    for rank, lam in ((50, 0.01), (128, 1e-6), (3, 0.01)):
        Y = ref.item_block(C.shape[1], rank)
        X = ref.item_block(C.shape[0], rank, seed=1)
        got = ops.ials_loss(device_matrix(ops, 'wide'), strided(ops, X), strided(ops, Y, 5, 2), lam)
        want = ref.objective(C, X, Y, lam)
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
        assert abs(ref.objective_by_traces(C, X, Y, lam) - want) <= 1e-12 * abs(want)


@functools.lru_cache(maxsize=None)
def built_model(ops, name):
    m = ref.model_for(ref.model_case(name), ops, compute_loss=True)
    m.build()
    return m


@pytest.mark.parametrize('name', list(ref.MODEL_CASES))
def test_model_matches_the_restated_fit(hip_ops, name):
    case = ref.model_case(name)
    m = built_model(hip_ops, name)
    X, Y = m.factors['userid'], m.factors['itemid']
    assert m.method == 'iALS' and X.shape == case['X'].shape and Y.shape == case['Y'].shape and X.dtype == Y.dtype == np.float64
    dist = max(ref.rel_distance(X, case['X']), ref.rel_distance(Y, case['Y']))
    print('model %s: d = %.3g, device distance = %.3g (%.2f d)' % (name, case['d'], dist, dist / case['d']))
    assert 0 < case['d'] < 1e-12
    assert dist <= 16 * case['d'], (dist, case['d'])
    assert np.array_equal(m._get_test_data()[2], case['test_users'])
    recs = m.get_recommendations()
    assert recs.dtype == np.int64
    ref.check_lists(recs, case['lists'], case['gaps'])
    loss = np.array(m.loss_history)
    assert len(loss) == 2 * case['epochs'] == len(case['loss']) and len(m.iterations_time) == case['epochs']
    assert (loss[1:] <= loss[:-1] * (1 + 1e-12)).all()
    assert np.allclose(loss, case['loss'], rtol=1e-9, atol=0)
    s, _ = m.slice_recommendations(*m._get_test_data()[:2], 0, 5, m._get_test_data()[2])
    assert np.allclose(s, case['X'][case['test_users'][:5]] @ case['Y'].T, rtol=0, atol=1e-10)


def test_warm_start_folds_the_test_users_in(hip_ops):
    ops = hip_ops
    w = ref.warm_case()
    case = w['case']
    m = ref.model_for(case, ops, data=ref.warm_data(w))
    m.build()
    assert ref.rel_distance(m.factors['itemid'], case['Y']) <= 16 * case['d']
    with pytest.raises(ValueError, match='The model always filters seen items from results.'):
        m.filter_seen = False
        m.get_recommendations()
    m.filter_seen = True
    tu, ti, tf = w['test']
    keep = tf != 1.0
    assert (~keep).sum() >= w['n_new']
    import scipy.sparse as sps
    Cw = sps.csr_matrix((np.log2(tf[keep]), (tu[keep], ti[keep])), shape=(w['n_new'], case['n_items']))
    Cw.sort_indices()
    folded = m.fold_in_matrix()
    assert folded.nnz == Cw.nnz and np.array_equal(ops.to_host(folded.indices), Cw.indices) and np.array_equal(ops.to_host(folded.values), Cw.data)
    Yd, Gd = m._item_factors_block()
    Y, G = ops.to_host(Yd), ops.to_host(Gd)
    assert np.array_equal(Y, m.factors['itemid'])
    got = ops.to_host(m.fold_in())
    want = ref.half_step(Cw, Y, G, ref.LAMBDA)
    bounds = ref.row_bounds(Cw, Y, G, ref.LAMBDA, want)
    assert ref.dropped_interaction_margin(Cw, Y, G, ref.LAMBDA, want, bounds) >= DROPPED_MARGIN
    err = np.linalg.norm(got - want, axis=1)
    folded_rows = bounds > 0                                             # a user whose known feedback is all 1 has nothing to fold in
    assert folded_rows.sum() >= w['n_new'] - 3 and not got[~folded_rows].any()
    print('fold-in: largest error / bound = %.3g' % (err[folded_rows] / bounds[folded_rows]).max())
    assert (err <= bounds).all()
    recs = m.get_recommendations()
    lists, gaps = ref.lists_and_gaps(want @ Y.T, (tu, ti))                # every test entry is seen, the confidence-0 ones too
    ref.check_lists(recs, lists, gaps)
    unseen_lists, _ = ref.lists_and_gaps(want @ Y.T, (tu[keep], ti[keep]))
    assert not np.array_equal(unseen_lists, lists)                        # masking the confidence-0 entries matters here
    for u in range(w['n_new']):
        assert not set(recs[u]) & set(ti[tu == u])
    s, _ = m.slice_recommendations(*m._get_test_data()[:2], 3, 9, m._get_test_data()[2])
    assert np.allclose(s, want[3:9] @ Y.T, rtol=0, atol=1e-10)


def test_scaled_composition_and_identical_builds(hip_ops):
    class ScaledIALS(ScaledMatrixMixin, ials.ImplicitALS):
        pass
    case = ref.model_case('r16')
    plain = built_model(hip_ops, 'r16')
    runs = []
    for _ in range(2):
        m = ref.model_for(case, hip_ops, cls=ScaledIALS)
        m.epsilon = 0.25                        # scaled values are < 1: keep every confidence log2(v / epsilon) positive
        m.build()
        runs.append((m.factors['userid'].copy(), m.factors['itemid'].copy(), m.get_recommendations().copy()))
    assert m.method == 'iALS-s'
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    unscaled = ref.model_for(case, hip_ops)
    unscaled.epsilon = 0.25
    unscaled.build()
    assert ref.rel_distance(runs[0][0], unscaled.factors['userid']) > 1e-3       # the same confidence transform, unscaled values
    again = ref.model_for(case, hip_ops)
    again.build()
    assert again.factors['userid'].tobytes() == plain.factors['userid'].tobytes()
    assert again.factors['itemid'].tobytes() == plain.factors['itemid'].tobytes()
