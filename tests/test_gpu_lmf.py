"""Logistic matrix factorisation on the device: the draw stream and the half-step kernel (csrc/lmf.hip) against the NumPy
restatement (tests/lmf_reference.py) BIT FOR BIT — the specification fixes the order of every sum —, its independence of the row
order, an epoch pair chained on the device, and the model — standard scenario, warm start, the scaled composition — against the
restated fit."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import lmf_reference as ref
from polara_amd import lmf
from polara_amd.models import ScaledMatrixMixin
from sweep_helpers import padding_is_zero, same_bits, strided

pytestmark = pytest.mark.gpu

# K = rank + 2 on both sides of every instance boundary (the padded widths 16, 32, .. 128), the smallest and the largest
RANKS = [1, 3, 13, 14, 15, 30, 31, 46, 47, 62, 63, 78, 79, 94, 95, 110, 111, 126]
LR, REG = 1.0, 0.6


def device_csr(ops, C):
    return ops.csr(C.indptr, C.indices, np.asarray(C.data, dtype=np.float64), C.shape)


@functools.lru_cache(maxsize=None)
def device_matrix(ops, kind):
    return device_csr(ops, ref.confidence_matrix(kind))


def check_half_step(ops, kind, rank, neg_prop, side, pad=0, seed=7, rnd=3):
    """one half-step on the device against the restatement: the same bits in X and in A"""
    C = ref.confidence_matrix(kind)
    X, A, Y, pinned = ref.blocks(C.shape[0], C.shape[1], rank, side)
    plan = ops.lmf_plan(device_matrix(ops, kind), neg_prop)
    if pad:
        Xd, Ad, Yd = strided(ops, X, pad, 1), strided(ops, A, pad + 1, 2), strided(ops, Y, pad + 2, 0)
        assert Xd.stride(0) > rank + 2 and Ad.stride(0) > Xd.stride(0) and Yd.stride(0) > Ad.stride(0)
    else:
        Xd, Ad, Yd = ops.to_device(X), ops.to_device(A), ops.to_device(Y)
    assert ops.lmf_half_step(plan, Yd, Xd, Ad, LR, REG, seed, rnd, pinned) is Xd
    want_x, want_a = ref.half_step(C, Y, X, A, LR, REG, neg_prop, seed, rnd, pinned)
    got_x, got_a = ops.to_host(Xd), ops.to_host(Ad)
    assert same_bits(got_x, want_x) and same_bits(got_a, want_a)
    assert same_bits(ops.to_host(Yd), Y)
    empty = np.diff(C.indptr) == 0
    assert empty.any() and same_bits(got_x[empty], X[empty]) and same_bits(got_x[:, pinned], X[:, pinned])
    assert not same_bits(got_x[~empty], X[~empty])
    if pad:
        assert padding_is_zero(Xd) and padding_is_zero(Ad) and padding_is_zero(Yd)        # nothing written beside the rows


def test_draws_equal_the_restatement(hip_ops):
    ops = hip_ops
    C = ref.confidence_matrix('wide')
    for neg_prop, seed, rnd in ((3, 5, 2), (1, 2 ** 32 - 1, ref.FOLD_IN_ROUND | 1), (30, 0, 0)):
        plan = ops.lmf_plan(device_matrix(ops, 'wide'), neg_prop)
        ptr = ref.neg_pointers(C.indptr, C.shape[1], neg_prop)
        assert np.array_equal(ops.to_host(plan['neg_ptr']), ptr) and plan['negatives'] == ptr[-1]
        assert plan is ops.lmf_plan(device_matrix(ops, 'wide'), neg_prop)                     # kept on the matrix
        got = ops.to_host(ops.lmf_draw_negatives(plan, seed, rnd))
        assert got.dtype == np.int32 and np.array_equal(got, ref.draw_negatives(C, neg_prop, seed, rnd))
    long_row = ref.WIDE_LENGTHS.index(1000)
    ptr = ref.neg_pointers(C.indptr, C.shape[1], 3)
    assert ptr[long_row + 1] - ptr[long_row] == C.shape[1] < 3000                              # the row where the cap binds
    order = ops.to_host(ops.lmf_plan(device_matrix(ops, 'wide'), 3)['row_order'])
    assert order[0] == long_row and sorted(order) == list(range(C.shape[0]))


@pytest.mark.parametrize('neg_prop', [1, 3])
@pytest.mark.parametrize('side', ['user', 'item'])
@pytest.mark.parametrize('rank', RANKS)
def test_half_step_equals_the_restatement_bit_for_bit(hip_ops, rank, side, neg_prop):
    """40 rows x 1 100 columns; row lengths 0 .. 9 around PK_LMF_CHAINS, 15 .. 17, 31 .. 33 and 63 .. 65 around the staging chunks
    (whose length depends on the instance), 257 (several chunks) and 1 000 (with neg_prop 3 the cap binds); every rank at which the
    kernel takes another instance, both pinned columns"""
    check_half_step(hip_ops, 'wide', rank, neg_prop, side)


@pytest.mark.parametrize('rank, side', [(3, 'user'), (30, 'item'), (47, 'user'), (126, 'item')])
def test_half_step_honours_leading_dimensions(hip_ops, rank, side):
    check_half_step(hip_ops, 'wide', rank, 3, side, pad=3)


def test_half_step_with_more_rows_than_one_wave_of_workgroups(hip_ops):
    check_half_step(hip_ops, 'tall', 5, 3, 'user')
    check_half_step(hip_ops, 'tall', 20, 1, 'item')


def test_half_step_is_deterministic_and_independent_of_the_row_order(hip_ops):
    ops = hip_ops
    for kind, rank in (('wide', 50), ('tall', 5)):
        Cd = device_matrix(ops, kind)
        plan = ops.lmf_plan(Cd, 3)
        X, A, Y, pinned = ref.blocks(Cd.shape[0], Cd.shape[1], rank, 'user')
        Yd = ops.to_device(Y)
        order = plan['row_order']
        lengths = np.diff(ops.to_host(Cd.indptr))[ops.to_host(order)]
        assert (np.diff(lengths) <= 0).all()                                                  # longest rows first
        runs = []
        for row_order in (None, None, torch.flip(order, [0]).contiguous()):
            Xd, Ad = ops.to_device(X), ops.to_device(A)
            ops.lmf_half_step(plan, Yd, Xd, Ad, LR, REG, 1, 0, pinned, row_order=row_order)
            runs.append((ops.to_host(Xd).tobytes(), ops.to_host(Ad).tobytes()))
        assert runs[0] == runs[1] == runs[2]


def test_an_epoch_pair_chained_on_the_device(hip_ops):
    ops = hip_ops
    C = ref.confidence_matrix('wide')
    Ct = sps.csr_matrix(C.T)
    Ct.sort_indices()
    Cd = device_matrix(ops, 'wide')
    rank, neg_prop, seed = 14, 3, 11
    K = rank + 2
    X, AX, Y, _ = ref.blocks(C.shape[0], C.shape[1], rank, 'user')
    AY = np.zeros_like(Y)
    Xd, AXd, Yd, AYd = (ops.to_device(a) for a in (X, AX, Y, AY))
    users, items = ops.lmf_plan(Cd, neg_prop), ops.lmf_plan(Cd.T, neg_prop)
    assert items['negatives'] == ref.neg_pointers(Ct.indptr, C.shape[0], neg_prop)[-1]
    for epoch in range(2):
        ops.lmf_half_step(users, Yd, Xd, AXd, LR, REG, seed, 2 * epoch, K - 1)
        ops.lmf_half_step(items, Xd, Yd, AYd, LR, REG, seed, 2 * epoch + 1, K - 2)
        X, AX = ref.half_step(C, Y, X, AX, LR, REG, neg_prop, seed, 2 * epoch, K - 1)
        Y, AY = ref.half_step(Ct, X, Y, AY, LR, REG, neg_prop, seed, 2 * epoch + 1, K - 2)
    for got, want in ((Xd, X), (AXd, AX), (Yd, Y), (AYd, AY)):
        assert same_bits(ops.to_host(got), want)


def test_half_step_checks_its_arguments(hip_ops):
    ops = hip_ops
    Cd = device_matrix(ops, 'tall')
    plan = ops.lmf_plan(Cd, 2)
    n, top = Cd.shape[0], ops.lmf_max_rank()
    assert top == ref.MAX_RANK == 126 and ops.lib.pk_lmf_chains() == ref.CHAINS
    with pytest.raises(ValueError, match='rank %d' % (top + 1)):
        ops.lmf_half_step(plan, ops.zeros(16, top + 3), ops.zeros(n, top + 3), ops.zeros(n, top + 3), LR, REG, 0, 0, 0)
    with pytest.raises(ValueError, match='block of shape'):
        ops.lmf_half_step(plan, ops.zeros(15, 6), ops.zeros(n, 6), ops.zeros(n, 6), LR, REG, 0, 0, 5)
    with pytest.raises(ValueError, match='block of shape'):
        ops.lmf_half_step(plan, ops.zeros(16, 6), ops.zeros(n, 6), ops.zeros(n - 1, 6), LR, REG, 0, 0, 5)
    with pytest.raises(ValueError, match='pinned'):
        ops.lmf_half_step(plan, ops.zeros(16, 6), ops.zeros(n, 6), ops.zeros(n, 6), LR, REG, 0, 0, 6)
    with pytest.raises(ValueError, match='32 unsigned bits'):
        ops.lmf_half_step(plan, ops.zeros(16, 6), ops.zeros(n, 6), ops.zeros(n, 6), LR, REG, 2 ** 32, 0, 5)
    with pytest.raises(ValueError, match='row_order'):
        ops.lmf_half_step(plan, ops.zeros(16, 6), ops.zeros(n, 6), ops.zeros(n, 6), LR, REG, 0, 0, 5,
                          row_order=torch.arange(n, device=ops.device))
    with pytest.raises(ValueError, match='neg_prop'):
        ops.lmf_plan(Cd, 0)


# ---- the model -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built_model(ops, name):
    m = ref.model_for(ref.model_case(name), ops)
    m.build()
    return m


@pytest.mark.parametrize('name', list(ref.MODEL_CASES))
def test_model_equals_the_restated_fit(hip_ops, name):
    case = ref.model_case(name)
    m = built_model(hip_ops, name)
    X, Y = m.factors['userid'], m.factors['itemid']
    assert m.method == 'LMF' and same_bits(X, np.asarray(case['X'])) and same_bits(Y, np.asarray(case['Y']))
    C, Ct = case['C'], sps.csr_matrix(case['C'].T)
    assert m.build_stats == dict(seed=case['seed'], epochs=case['epochs'], neg_prop=case['neg_prop'],
                                 user_negatives=int(ref.neg_pointers(C.indptr, C.shape[1], case['neg_prop'])[-1]),
                                 item_negatives=int(ref.neg_pointers(Ct.indptr, C.shape[0], case['neg_prop'])[-1]))
    assert len(m.iterations_time) == case['epochs'] and np.array_equal(m._get_test_data()[2], case['test_users'])
    recs = m.get_recommendations()
    assert recs.dtype == np.int64
    ref.check_lists(recs, case['lists'], case['gaps'])
    s, _ = m.slice_recommendations(*m._get_test_data()[:2], 0, 5, m._get_test_data()[2])
    assert np.allclose(s, case['X'][case['test_users'][:5]] @ case['Y'].T, rtol=0, atol=1e-10)


def test_warm_start_folds_the_test_users_in(hip_ops):
    ops = hip_ops
    w = ref.warm_case()
    case = w['case']
    m = ref.model_for(case, ops, data=ref.warm_data(w))
    m.fold_in_epochs = 4
    m.build()
    assert same_bits(m.factors['itemid'], np.asarray(case['Y']))
    with pytest.raises(ValueError, match='The model always filters seen items from results.'):
        m.filter_seen = False
        m.get_recommendations()
    m.filter_seen = True
    tu, ti, tf = w['test']
    keep = tf != 1.0
    assert (~keep).sum() >= w['n_new']
    Cw = sps.csr_matrix((np.log2(tf[keep]), (tu[keep], ti[keep])), shape=(w['n_new'], case['n_items']))
    Cw.sort_indices()
    folded = m.fold_in_matrix()
    assert folded.nnz == Cw.nnz and np.array_equal(ops.to_host(folded.indices), Cw.indices) and np.array_equal(ops.to_host(folded.values), Cw.data)
    want = ref.fold_in(Cw, np.asarray(case['Y']), ref.LEARNING_RATE, ref.REGULARIZATION, case['neg_prop'], case['seed'], 4)
    got = ops.to_host(m.fold_in())
    assert same_bits(got, want) and m.fold_in().stride(0) % 2 == 0
    recs = m.get_recommendations()
    lists, gaps = ref.lists_and_gaps(want @ case['Y'].T, (tu, ti))                # every test entry is seen, the confidence-0 ones too
    ref.check_lists(recs, lists, gaps)
    for u in range(w['n_new']):
        assert not set(recs[u]) & set(ti[tu == u])
    s, _ = m.slice_recommendations(*m._get_test_data()[:2], 3, 9, m._get_test_data()[2])
    assert np.allclose(s, want[3:9] @ case['Y'].T, rtol=0, atol=1e-10)


def test_scaled_composition_and_identical_builds(hip_ops):
    class ScaledLMF(ScaledMatrixMixin, lmf.ImplicitLMF):
        pass
    case = ref.model_case('r14')
    plain = built_model(hip_ops, 'r14')
    runs = []
    for _ in range(2):
        m = ref.model_for(case, hip_ops, cls=ScaledLMF)
        m.epsilon = 0.25                        # scaled values are < 1: keep every confidence log2(v / epsilon) positive
        m.build()
        runs.append((m.factors['userid'].copy(), m.factors['itemid'].copy(), m.get_recommendations().copy()))
    assert m.method == 'LMF-s'
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    # the restated fit on the confidences the scaled model was given
    scaled = m.get_training_matrix()
    scaled.sort_indices()
    Cs = sps.csr_matrix((np.log2(scaled.data / 0.25), scaled.indices, scaled.indptr), shape=scaled.shape)
    Cd = m._confidence_csr(m._training_device_csr())
    assert np.array_equal(hip_ops.to_host(Cd.indices), Cs.indices)
    Cs.data = hip_ops.to_host(Cd.values)                                      # the device's own scaling arithmetic: only the solver is under test
    Xs, Ys = ref.fit(Cs, case['rank'], ref.LEARNING_RATE, ref.REGULARIZATION, case['neg_prop'], case['epochs'], case['seed'])
    assert same_bits(runs[0][0], Xs) and same_bits(runs[0][1], Ys)
    assert ref.rel_distance(runs[0][0], plain.factors['userid']) > 1e-3
    again = ref.model_for(case, hip_ops)
    again.build()
    assert again.factors['userid'].tobytes() == plain.factors['userid'].tobytes()
    assert again.factors['itemid'].tobytes() == plain.factors['itemid'].tobytes()
