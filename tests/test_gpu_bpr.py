"""BPR on the device: the sigmoid, the plan, the negatives and one epoch of the sweep kernel (csrc/bpr.hip) against the NumPy
restatement (tests/bpr_reference.py) BIT FOR BIT, and the full model against the restated fit."""
import functools

import numpy as np
import pytest
import torch

import bpr_reference as ref
from polara_amd import bpr  # noqa: F401  (the module under test: without it nothing here can run)
from sweep_helpers import (MANY_STRATA_BLOCKS, MANY_STRATA_SEED, device_csr, many_strata_matrix, padding_is_zero, same_bits, strided,
                           trained_in_the_last_stratum)
from test_bpr_host import (FORWARDING_SEED, GRID, LEARN, POINTS, check_model_against_the_restated_fit, check_model_refusals,
                           planted_model)

pytestmark = pytest.mark.gpu

LR, REG = 0.05, 0.01
PLAN_KEYS = ('perm', 'block_ptr', 'item_ptr', 'users', 'items', 'item_order', 'item_part')


@functools.lru_cache(maxsize=None)
def restated_epoch(case, blocks, rank):
    """(dense, order, seed, plan, neg, P0, Q0, P, Q, counts) of one restated epoch: computed once per case, never written to"""
    if case == 'forwarding':
        dense, seed = ref.forwarding_matrix(), FORWARDING_SEED
        order = ref.item_order(seed, 0, dense.shape[1])
    elif case == 'corner':
        (dense, order), seed = ref.corner_matrix(), 5
    elif case == 'many strata':
        dense, seed = many_strata_matrix(), MANY_STRATA_SEED
        order = ref.item_order(seed, 0, dense.shape[1])
    else:
        dense, seed = ref.random_matrix(), 100 * blocks + rank
        order = ref.item_order(seed, 0, dense.shape[1])
    plan = ref.make_plan(dense, blocks, order)
    neg = ref.draw_negatives(plan, seed, 0)
    P0, Q0 = ref.initial_factors(dense.shape[0], dense.shape[1], rank, seed)
    Q0[:, rank] = np.random.RandomState(seed).normal(scale=0.1, size=dense.shape[1])      # a bias that is not zero
    P, Q = P0.copy(), Q0.copy()
    counts = ref.epoch(plan, neg, P, Q, LR, REG)
    for a in (dense, order, neg, P0, Q0, P, Q) + tuple(plan[k] for k in PLAN_KEYS):
        a.setflags(write=False)
    return dense, order, seed, plan, neg, P0, Q0, P, Q, counts


def check_plan_and_negatives(ops, case, blocks):
    dense, order, seed, host, neg = restated_epoch(case, blocks, 7)[:5]
    dev = ops.bpr_plan(device_csr(ops, dense), blocks, order)
    assert dev['blocks'] == blocks and dev['nnz'] == host['nnz'] and dev['shape'] == host['shape']
    for key in PLAN_KEYS:
        got = ops.to_host(dev[key])
        assert got.dtype == host[key].dtype and np.array_equal(got, host[key]), key
    got = ops.to_host(ops.bpr_draw_negatives(dev, seed, 0))
    assert got.dtype == np.int32 and np.array_equal(got, neg)
    return dev, neg


def run_epoch(ops, case, blocks, rank):
    dense, order, seed, host, neg, P0, Q0, P, Q, counts = restated_epoch(case, blocks, rank)
    plan = ops.bpr_plan(device_csr(ops, dense), blocks, order)
    neg_dev = ops.bpr_draw_negatives(plan, seed, 0)
    assert np.array_equal(ops.to_host(neg_dev), neg)
    Pd, Qd = strided(ops, P0, 3, 1), strided(ops, Q0, 5, 2)
    out = ops.bpr_epoch(plan, neg_dev, Pd, Qd, LR, REG)
    assert out.dtype == torch.int64 and tuple(out.shape) == (3,)
    assert tuple(int(c) for c in ops.to_host(out)) == counts
    assert same_bits(ops.to_host(Pd), P) and same_bits(ops.to_host(Qd), Q)
    assert padding_is_zero(Pd) and padding_is_zero(Qd)
    assert counts[0] + counts[1] == host['nnz']
    return counts


# ---- the sigmoid ---------------------------------------------------------------------------------------------------------------
def test_sigmoid_is_bit_equal_to_the_restatement(hip_ops):
    for x in (GRID, POINTS):
        got = hip_ops.to_host(hip_ops.bpr_sigmoid(hip_ops.to_device(x)))
        assert same_bits(got, ref.sigmoid(x))
    edge = hip_ops.to_host(hip_ops.bpr_sigmoid(hip_ops.to_device(POINTS[6:])))
    assert edge[0] == 0.0 and edge[1] == 1.0 and np.isnan(edge[2])


# ---- plan and negatives ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', [1, 2, 5])
def test_device_plan_and_negatives_equal_the_restatement(hip_ops, blocks):
    dev, neg = check_plan_and_negatives(hip_ops, 'random', blocks)
    assert not np.array_equal(hip_ops.to_host(dev['item_order']), np.arange(23)) and (neg >= 0).any()


def test_device_negatives_of_the_skip_corners(hip_ops):
    dev, neg = check_plan_and_negatives(hip_ops, 'corner', 2)
    items, users = hip_ops.to_host(dev['items']), hip_ops.to_host(dev['users'])
    assert np.array_equal(hip_ops.to_host(dev['item_ptr']), [0, 1, 6])
    assert (neg[items == 0] == -1).all() and (neg[users == 0] == -1).all() and (neg >= 0).sum() == 2


def test_device_plan_with_the_identity_order_is_pmfs(hip_ops):
    A = device_csr(hip_ops, ref.random_matrix())
    got, want = hip_ops.bpr_plan(A, 5), hip_ops.pmf_plan(A, 5)
    for key in ('perm', 'block_ptr', 'users', 'items'):
        assert torch.equal(got[key], want[key]), key
    assert np.array_equal(hip_ops.to_host(got['item_order']), np.arange(23))


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rank', [1, 7, 15, 16, 31, 63])
@pytest.mark.parametrize('blocks', [1, 2, 5])
def test_one_epoch_is_bit_equal_to_the_restatement(hip_ops, blocks, rank):
    """k + 1 = 2, 8, 16 (lane groups of 16), 17, 32 (of 32), 64 (a full wave); one block per launch, fewer blocks than a wave holds
    and — at width 64 — more than one workgroup; P and Q with leading dimensions of their own"""
    counts = run_epoch(hip_ops, 'random', blocks, rank)
    assert counts[0] > 0


def test_the_forwarding_case_is_bit_equal(hip_ops):
    """consecutive samples that share the user, the negative, swap positive and negative, or share the positive"""
    neg, items = restated_epoch('forwarding', 1, 3)[4], restated_epoch('forwarding', 1, 3)[3]['items']
    assert neg[2] == items[3] and neg[3] == items[2] and neg[0] == neg[1] and items[4] == items[5]
    assert run_epoch(hip_ops, 'forwarding', 1, 3)[:2] == (6, 0)


def test_the_skip_corners_are_bit_equal(hip_ops):
    assert run_epoch(hip_ops, 'corner', 2, 3)[:2] == (2, 13)


def test_more_strata_than_the_counters_reduction_has_threads(hip_ops):
    """B = 257: the reduction of the block counters strides the strata over 256 threads, so stratum 256 is its second trip.  By
    the restatement alone a sample of that stratum is trained (a wrong trip would lose it) and some samples are skipped."""
    plan, neg = restated_epoch('many strata', MANY_STRATA_BLOCKS, 1)[3:5]
    assert trained_in_the_last_stratum(plan, neg >= 0) and (neg < 0).any()
    trained, skipped, _ = run_epoch(hip_ops, 'many strata', MANY_STRATA_BLOCKS, 1)
    assert trained > 0 and skipped > 0


def test_a_second_epoch_continues_from_the_first(hip_ops):
    """two epochs on the device against two restated ones, the state staying on the device"""
    ops = hip_ops
    dense, seed = ref.random_matrix(), 21
    A = device_csr(ops, dense)
    P, Q = ref.initial_factors(37, 23, 10, seed)
    Pd, Qd = ops.to_device(P), ops.to_device(Q)
    for ep in range(2):
        order = ref.item_order(seed, ep, 23)
        host = ref.make_plan(dense, 4, order)
        want = ref.epoch(host, ref.draw_negatives(host, seed, ep), P, Q, LR, REG)
        plan = ops.bpr_plan(A, 4, order)
        got = ops.to_host(ops.bpr_epoch(plan, ops.bpr_draw_negatives(plan, seed, ep), Pd, Qd, LR, REG))
        assert tuple(int(c) for c in got) == want
    assert same_bits(ops.to_host(Pd), P) and same_bits(ops.to_host(Qd), Q)


def test_operators_check_their_arguments(hip_ops):
    ops = hip_ops
    dense = ref.random_matrix()
    A = device_csr(ops, dense)
    for bad in (0, 24):
        with pytest.raises(ValueError, match='blocks'):
            ops.bpr_plan(A, bad)
    with pytest.raises(ValueError, match='permutation'):
        ops.bpr_plan(A, 2, np.zeros(23, dtype=np.int64))
    plan = ops.bpr_plan(A, 2)
    neg = ops.bpr_draw_negatives(plan, 1, 0)
    max_rank = ops.bpr_max_rank()
    assert max_rank == ref.MAX_RANK == 63
    with pytest.raises(ValueError, match='rank 64'):
        ops.bpr_epoch(plan, neg, ops.zeros(37, 65), ops.zeros(23, 65), LR, REG)
    with pytest.raises(ValueError, match='block of shape'):
        ops.bpr_epoch(plan, neg, ops.zeros(36, 4), ops.zeros(23, 4), LR, REG)
    with pytest.raises(ValueError, match='block of shape'):
        ops.bpr_epoch(plan, neg, ops.zeros(37, 4), ops.zeros(23, 4, dtype=torch.float32), LR, REG)
    with pytest.raises(ValueError, match='negatives'):
        ops.bpr_epoch(plan, neg[:-1], ops.zeros(37, 4), ops.zeros(23, 4), LR, REG)
    with pytest.raises(ValueError, match='32 unsigned bits'):
        ops.bpr_draw_negatives(plan, 2 ** 32, 0)
    # the C entry refuses a rank above its bound with an error code, whatever the host layer checked
    P = ops.zeros(37, 66)
    rc = ops.lib.pk_bpr_epoch_f64(ops.stream(), 2, 64, plan['nnz'], plan['block_ptr'].data_ptr(), plan['users'].data_ptr(),
                                  plan['items'].data_ptr(), neg.data_ptr(), P.data_ptr(), P.stride(0), P.data_ptr() + 8, P.stride(0),
                                  LR, REG, ops.empty(12).data_ptr(), ops.empty(3).data_ptr())
    assert rc == -1 and b'rank' in ops.lib.pk_last_error()            # PK_E_INVALID


# ---- the model -------------------------------------------------------------------------------------------------------------------
def test_model_equals_the_restated_fit(hip_ops):
    check_model_against_the_restated_fit(planted_model(hip_ops))


def test_two_identical_builds_give_identical_bits_and_another_seed_other_factors(hip_ops):
    runs = []
    for seed in (LEARN['seed'], LEARN['seed'], LEARN['seed'] + 1):
        m = planted_model(hip_ops, random_state=seed, num_epochs=3)
        m.build()
        runs.append((m.factors['userid'], m.factors['itemid'], np.array(m.auc_history), m.get_recommendations()))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    assert not np.array_equal(runs[0][0], runs[2][0]) and not np.array_equal(runs[0][1], runs[2][1])


def test_model_refusals(hip_ops):
    check_model_refusals(planted_model(hip_ops, num_epochs=1))
