"""Probabilistic matrix factorisation on the device: the device plan against the host plan, one epoch of the sweep kernel
(csrc/pmf.hip) against the NumPy restatement (tests/pmf_reference.py) BIT FOR BIT — factors, adjuster state and squared
error — and the full model against the reference's fixtures (tests/golden/pmf_*.npz) at 4 x restatement_gap."""
import functools

import numpy as np
import pytest
import torch

import pmf_reference as ref
from conftest import load_golden
from polara_amd import pmf
from sweep_helpers import padding_is_zero, strided
from test_pmf_host import FIXTURES, check_pmf_model_against_fixture, interactions, restated_solution

pytestmark = pytest.mark.gpu

ETA, LAMBD = 0.05, 0.5


def fixture_triplets():
    g = load_golden('pmf_std')
    return g['train_idx'][:, 0], g['train_idx'][:, 1], g['train_val'], int(g['train_shape'][0]), int(g['train_shape'][1])


def tiny_triplets():
    """8 users x 8 items, 14 entries: with B = 4 user 0 (4 of 14 entries) is a part of its own, and several blocks hold one sample"""
    u = np.array([0, 0, 0, 0, 1, 2, 2, 3, 4, 5, 5, 6, 7, 7])
    i = np.array([0, 2, 5, 7, 1, 0, 3, 4, 6, 2, 7, 5, 1, 6])
    return u, i, np.arange(1., 15.), 8, 8


def device_csr(ops, u, i, v, n_users, n_items):
    return ops.csr_from_coo(u, i, np.asarray(v, dtype=np.float64), (n_users, n_items))


@functools.lru_cache(maxsize=None)
def restated_epoch(case, blocks, rank, adjust):
    """(P0, Q0, P, Q, SP, SQ, squared error) of one restated epoch: computed once per case, never written to"""
    u, i, v, n_users, n_items = tiny_triplets() if case == 'tiny' else fixture_triplets()
    plan = ref.make_plan(u, i, v, n_users, n_items, blocks)
    rng = np.random.RandomState(1000 * blocks + rank)
    P0, Q0 = rng.normal(scale=0.1, size=(n_users, rank)), rng.normal(scale=0.1, size=(n_items, rank))
    P, Q = P0.copy(), Q0.copy()
    S = (np.zeros_like(P), np.zeros_like(Q))
    sse = ref.epoch(plan, P, Q, ETA, LAMBD, adjust, S if adjust else None)
    out = (P0, Q0, P, Q, S[0], S[1], sse)
    for a in out[:6]:
        a.setflags(write=False)
    return out


def check_plan(ops, u, i, v, n_users, n_items, blocks):
    host = ref.make_plan(u, i, v, n_users, n_items, blocks)
    dev = ops.pmf_plan(device_csr(ops, u, i, v, n_users, n_items), blocks)
    assert dev['blocks'] == blocks and dev['nnz'] == len(u) and dev['shape'] == (n_users, n_items)
    for key in ('perm', 'block_ptr', 'users', 'items', 'vals', 'row_nnz', 'col_nnz'):
        got = ops.to_host(dev[key])
        assert got.dtype == host[key].dtype and np.array_equal(got, host[key]), key
    return host, dev


@pytest.mark.parametrize('blocks', [1, 4, 32, 150])
def test_device_plan_equals_host_plan(hip_ops, blocks):
    check_plan(hip_ops, *fixture_triplets(), blocks)


def test_device_plan_of_the_tiny_case_and_of_sparse_corners(hip_ops):
    u, i, v, n_users, n_items = tiny_triplets()
    host, _ = check_plan(hip_ops, u, i, v, n_users, n_items, 4)
    lengths = np.diff(host['block_ptr'])
    assert (lengths == 1).any() and (lengths == 0).any()                  # a block of one sample, empty blocks
    upart = pmf._parts(np.bincount(u, minlength=8), 4, len(u))
    assert (np.bincount(upart, minlength=4) == 1).any()                   # a part of one user
    check_plan(hip_ops, *interactions(9), 7)                              # users and items without interactions
    check_plan(hip_ops, *interactions(9), 30)                             # as many blocks as items


def test_device_plan_refuses_what_the_host_plan_refuses(hip_ops):
    u, i, v, n_users, n_items = tiny_triplets()
    A = device_csr(hip_ops, u, i, v, n_users, n_items)
    for bad in (0, 9):
        with pytest.raises(ValueError, match='blocks'):
            hip_ops.pmf_plan(A, bad)
    v0 = v.copy()
    v0[3] = 0.
    with pytest.raises(ValueError, match='feedback 0'):
        hip_ops.pmf_plan(device_csr(hip_ops, u, i, v0, n_users, n_items), 2)


def run_epoch(ops, case, blocks, rank, adjust):
    u, i, v, n_users, n_items = tiny_triplets() if case == 'tiny' else fixture_triplets()
    P0, Q0, P, Q, SP, SQ, sse = restated_epoch(case, blocks, rank, adjust)
    plan = ops.pmf_plan(device_csr(ops, u, i, v, n_users, n_items), blocks)
    Pd, Qd = strided(ops, P0), strided(ops, Q0, pad=5, off=2)
    state = (strided(ops, np.zeros_like(P0), pad=1, off=0), strided(ops, np.zeros_like(Q0), pad=2, off=2)) if adjust else None
    out = ops.pmf_epoch(plan, Pd, Qd, ETA, LAMBD, adjust=adjust, state=state)
    assert tuple(out.shape) == (1,)
    got_sse = float(out[0].item())
    assert np.array_equal(ops.to_host(Pd), P) and np.array_equal(ops.to_host(Qd), Q)
    assert got_sse == sse
    assert padding_is_zero(Pd) and padding_is_zero(Qd)
    if adjust:
        assert np.array_equal(ops.to_host(state[0]), SP) and np.array_equal(ops.to_host(state[1]), SQ)
        assert padding_is_zero(state[0]) and padding_is_zero(state[1])
    assert not np.array_equal(P, P0) and not np.array_equal(Q, Q0)


@pytest.mark.parametrize('adjust', [None, 'adagrad', 'rmsprop'])
@pytest.mark.parametrize('rank', [7, 10, 16, 17, 40, 64])
@pytest.mark.parametrize('blocks', [1, 4, 32])
def test_one_epoch_is_bit_equal_to_the_restatement(hip_ops, blocks, rank, adjust):
    """every lane-group width (16: ranks 7, 10, 16; 32: rank 17; 64: ranks 40, 64), full and partly idle groups, one block per
    launch (B = 1), fewer blocks than a wave holds (B = 4 at width 16) and more than one workgroup (B = 32); P, Q and the
    state with leading dimensions of their own"""
    run_epoch(hip_ops, 'fixture', blocks, rank, adjust)


@pytest.mark.parametrize('adjust', [None, 'adagrad', 'rmsprop'])
def test_the_tiny_case_is_bit_equal_to_the_restatement(hip_ops, adjust):
    run_epoch(hip_ops, 'tiny', 4, 3, adjust)


def test_a_second_epoch_continues_from_the_first(hip_ops):
    """two epochs on the device against two restated ones: the rows the first left in memory are what the second reads"""
    ops = hip_ops
    u, i, v, n_users, n_items = fixture_triplets()
    host = ref.make_plan(u, i, v, n_users, n_items, 16)
    plan = ops.pmf_plan(device_csr(ops, u, i, v, n_users, n_items), 16)
    rng = np.random.RandomState(5)
    P, Q = rng.normal(scale=0.1, size=(n_users, 10)), rng.normal(scale=0.1, size=(n_items, 10))
    Pd, Qd = ops.to_device(P), ops.to_device(Q)
    for _ in range(2):
        want = ref.epoch(host, P, Q, ETA, LAMBD)
        got = float(ops.pmf_epoch(plan, Pd, Qd, ETA, LAMBD)[0].item())
        assert got == want
    assert np.array_equal(ops.to_host(Pd), P) and np.array_equal(ops.to_host(Qd), Q)


def test_epoch_checks_its_arguments(hip_ops):
    ops = hip_ops
    u, i, v, n_users, n_items = tiny_triplets()
    plan = ops.pmf_plan(device_csr(ops, u, i, v, n_users, n_items), 2)
    max_rank = ops.pmf_max_rank()
    assert max_rank >= 64 and max_rank == ref.MAX_RANK
    with pytest.raises(ValueError, match='rank'):
        ops.pmf_epoch(plan, ops.zeros(8, max_rank + 1), ops.zeros(8, max_rank + 1), ETA, LAMBD)
    with pytest.raises(ValueError, match='block of shape'):
        ops.pmf_epoch(plan, ops.zeros(7, 3), ops.zeros(8, 3), ETA, LAMBD)
    with pytest.raises(ValueError, match='block of shape'):
        ops.pmf_epoch(plan, ops.zeros(8, 3), ops.zeros(8, 3, dtype=torch.float32), ETA, LAMBD)
    with pytest.raises(ValueError, match='state'):
        ops.pmf_epoch(plan, ops.zeros(8, 3), ops.zeros(8, 3), ETA, LAMBD, adjust='adagrad')
    with pytest.raises(ValueError, match='adjustment'):
        ops.pmf_epoch(plan, ops.zeros(8, 3), ops.zeros(8, 3), ETA, LAMBD, adjust='adam')
    # the C entry refuses a rank above its bound with an error code, whatever the host layer checked
    P = ops.zeros(8, max_rank + 1)
    rc = ops.lib.pk_pmf_epoch_f64(ops.stream(), 2, max_rank + 1, plan['nnz'], plan['block_ptr'].data_ptr(), plan['users'].data_ptr(),
                                  plan['items'].data_ptr(), plan['vals'].data_ptr(), P.data_ptr(), P.stride(0), P.data_ptr() + 8,
                                  P.stride(0), plan['row_nnz'].data_ptr(), plan['col_nnz'].data_ptr(), ETA, LAMBD, 0, None, 0, None, 0,
                                  0.9, 1e-6, ops.empty(4).data_ptr(), ops.empty(1).data_ptr())
    assert rc == -1 and b'rank' in ops.lib.pk_last_error()            # PK_E_INVALID


@pytest.mark.parametrize('name', FIXTURES)
def test_model_matches_the_reference(hip_ops, name):
    g = load_golden(name)
    m = ref.model_for(g, hip_ops)
    check_pmf_model_against_fixture(m, g)
    P, Q, history = restated_solution(name)                                # and the restatement bit for bit
    assert np.array_equal(m.factors['userid'], P) and np.array_equal(m.factors['itemid'], Q)
    assert np.array_equal(np.array(m.rmse_history), history)


def test_two_identical_builds_give_identical_bits(hip_ops):
    g = load_golden('pmf_rmsprop')
    runs = []
    for _ in range(2):
        m = ref.model_for(g, hip_ops)
        m.build(adjust_gradient='rmsprop')
        runs.append((m.factors['userid'].copy(), m.factors['itemid'].copy(), list(m.rmse_history), m.get_recommendations().copy()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_a_rank_above_the_bound_raises(hip_ops):
    g = load_golden('pmf_b4')
    m = ref.model_for(g, hip_ops)
    m.rank = hip_ops.pmf_max_rank() + 1
    with pytest.raises(ValueError, match='rank %d' % m.rank):
        m.build()
    assert not m._is_ready
