"""Kernelized PMF on the device: the device plan against the host plan, one epoch of the sweep kernel (csrc/kpmf.hip) against
the NumPy restatement (tests/kpmf_reference.py) BIT FOR BIT — factors, adjuster state, squared error and both snapshots — and
the full model against the reference's fixtures (tests/golden/kpmf_*.npz) at 4 x restatement_gap."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import kpmf_reference as ref
from conftest import load_golden
from sweep_helpers import padding_is_zero, strided
from test_gpu_pmf import device_csr, tiny_triplets
from test_kpmf_host import FIXTURES, check_kpmf_model_against_fixture, half_identity_kernels, restated_solution

pytestmark = pytest.mark.gpu

ETA, LAMBD = 0.05, 0.5
PLAN_KEYS = ('perm', 'block_ptr', 'users', 'items', 'vals', 'row_nnz', 'col_nnz', 'user_part', 'item_part', 'ku_ptr', 'ku_idx', 'ku_val',
             'ku_diag', 'ki_ptr', 'ki_idx', 'ki_val', 'ki_diag')


def fixture_case():
    g = load_golden('kpmf_std')
    return (g['train_idx'][:, 0], g['train_idx'][:, 1], g['train_val'], int(g['train_shape'][0]), int(g['train_shape'][1])) \
        + ref.fixture_kernels(g)


def tiny_case():
    """the 8 x 8 interactions of test_gpu_pmf.tiny_triplets at B = 4 — user parts [0, 1, 1, 2, 2, 2, 3, 3], item parts
    [0, 0, 1, 1, 2, 2, 2, 3] — with hand-made kernels (checked in test_the_tiny_case_holds_what_it_is_meant_to)"""
    u, i, v, n_users, n_items = tiny_triplets()
    Ku = np.zeros((8, 8))
    Ku[0, [0, 2, 5, 7]] = [1.1, 0.3, -0.2, 0.45]        # user 0 is a part of its own: every neighbour lies in another part
    Ku[1, 1] = 1.3                                      # only the diagonal
    Ku[2, [1, 2, 6]] = [0.7, 1.05, 0.15]                # user 1: own part, updated by the same block just before (block (1, 0))
    Ku[3, [3, 4]] = [0.9, 0.25]
    Ku[4, [0, 3]] = [0.35, -0.4]                        # no stored diagonal
    Ku[5, [5]] = [1.0]
    Ku[6, [6, 7, 0]] = [1.2, 0.5, 0.1]
    Ku[7, [6, 7]] = [0.5, 0.8]
    rng = np.random.RandomState(8)
    Ki = np.diag(1. + rng.rand(8))
    Ki[2] = 0.1 + rng.rand(8)                           # a full row: 7 neighbours — more than one batch of loads, and a tail
    Ki[0, [1, 5]] = [0.6, 0.2]                          # item 1: own part of item 0
    Ki[7, [2, 6]] = [0.3, 0.3]
    Ki[5, [4, 6, 0]] = [0.2, 0.4, 0.6]
    return u, i, v, n_users, n_items, sps.csr_matrix(Ku), sps.csr_matrix(Ki)


def case_of(name):
    return tiny_case() if name == 'tiny' else fixture_case()


@functools.lru_cache(maxsize=None)
def restated_epochs(case, blocks, rank, adjust, epochs=1):
    """(P0, Q0, P, Q, SP, SQ, squared errors) of `epochs` restated epochs (the state zeroed before each): computed once per
    case, never written to"""
    plan = ref.make_plan(*case_of(case)[:5], blocks, *case_of(case)[5:])
    n_users, n_items = plan['shape']
    rng = np.random.RandomState(1000 * blocks + rank)
    P0, Q0 = rng.normal(scale=0.1, size=(n_users, rank)), rng.normal(scale=0.1, size=(n_items, rank))
    P, Q = P0.copy(), Q0.copy()
    S = (np.zeros_like(P), np.zeros_like(Q))
    sse = []
    for _ in range(epochs):
        S[0][:], S[1][:] = 0., 0.
        sse.append(ref.epoch(plan, P, Q, ETA, LAMBD, adjust, S if adjust else None))
    out = (P0, Q0, P, Q, S[0], S[1], tuple(sse))
    for a in out[:6]:
        a.setflags(write=False)
    return out


def device_plan(ops, case, blocks):
    u, i, v, n_users, n_items, Ku, Ki = case_of(case)
    return ops.kpmf_plan(device_csr(ops, u, i, v, n_users, n_items), blocks, Ku, Ki)


@pytest.mark.parametrize('case, blocks', [('fixture', 1), ('fixture', 4), ('fixture', 32), ('tiny', 4)])
def test_device_plan_equals_host_plan(hip_ops, case, blocks):
    u, i, v, n_users, n_items, Ku, Ki = case_of(case)
    host = ref.make_plan(u, i, v, n_users, n_items, blocks, Ku, Ki)
    dev = device_plan(hip_ops, case, blocks)
    assert dev['blocks'] == blocks and dev['nnz'] == len(u) and dev['shape'] == (n_users, n_items)
    for key in PLAN_KEYS:
        got = hip_ops.to_host(dev[key])
        assert got.dtype == host[key].dtype and np.array_equal(got, host[key]), key


def test_the_tiny_case_holds_what_it_is_meant_to():
    """no device: the hand-made kernels really contain the rows the sweep must get right"""
    u, i, v, n_users, n_items, Ku, Ki = tiny_case()
    plan = ref.make_plan(u, i, v, n_users, n_items, 4, Ku, Ki)
    up, ip = plan['user_part'], plan['item_part']
    assert up.tolist() == [0, 1, 1, 2, 2, 2, 3, 3] and ip.tolist() == [0, 0, 1, 1, 2, 2, 2, 3]
    row = lambda side, r: plan[side + '_idx'][plan[side + '_ptr'][r]:plan[side + '_ptr'][r + 1]]
    assert len(row('ku', 1)) == 0 and plan['ku_diag'][1] != 0                           # a row with only its diagonal
    assert plan['ku_diag'][4] == 0 and len(row('ku', 4)) == 2                           # a row without a stored diagonal
    assert len(row('ku', 0)) == 3 and (up[row('ku', 0)] != up[0]).all()                 # all neighbours in other parts
    assert row('ki', 2).tolist() == [0, 1, 3, 4, 5, 6, 7]                               # a full row: one batch of 4 and a tail of 3
    # user 2 reads user 1 live, and block (1, 0) of stratum 3 updates user 1 just before it comes to user 2
    assert 1 in row('ku', 2) and up[1] == up[2] == 1
    s, b = 3, 1
    lo, hi = plan['block_ptr'][s * 4 + b], plan['block_ptr'][s * 4 + b + 1]
    assert plan['users'][lo:hi].tolist() == [1, 2] and (ip[plan['items'][lo:hi]] == (b + s) % 4).all()
    # ... so live and snapshot reads differ on this case
    rng = np.random.RandomState(0)
    P0, Q0 = rng.normal(scale=0.1, size=(8, 3)), rng.normal(scale=0.1, size=(8, 3))
    P, Q, sP, sQ = P0.copy(), Q0.copy(), P0.copy(), Q0.copy()
    ref.epoch(plan, P, Q, ETA, LAMBD)
    ref.epoch(plan, sP, sQ, ETA, LAMBD, live=False)
    assert not np.array_equal(P[2], sP[2]) and not np.array_equal(Q, sQ)


def run_epochs(ops, case, blocks, rank, adjust, epochs=1):
    P0, Q0, P, Q, SP, SQ, sse = restated_epochs(case, blocks, rank, adjust, epochs)
    plan = device_plan(ops, case, blocks)
    Pd, Qd = strided(ops, P0), strided(ops, Q0, pad=5, off=2)
    snaps = (strided(ops, np.zeros_like(P0), pad=2, off=1), strided(ops, np.zeros_like(Q0), pad=1, off=0))
    state = (strided(ops, np.zeros_like(P0), pad=1, off=0), strided(ops, np.zeros_like(Q0), pad=2, off=2)) if adjust else None
    for e in range(epochs):
        if adjust:
            state[0].zero_()
            state[1].zero_()
        out = ops.kpmf_epoch(plan, Pd, Qd, ETA, LAMBD, adjust=adjust, state=state, snapshots=snaps)
        assert tuple(out.shape) == (1,)
        assert float(out[0].item()) == sse[e]
    assert np.array_equal(ops.to_host(Pd), P) and np.array_equal(ops.to_host(Qd), Q)
    assert np.array_equal(ops.to_host(snaps[0]), P) and np.array_equal(ops.to_host(snaps[1]), Q)     # what the last stratum left
    assert all(padding_is_zero(x) for x in (Pd, Qd) + snaps)
    if adjust:
        assert np.array_equal(ops.to_host(state[0]), SP) and np.array_equal(ops.to_host(state[1]), SQ)
        assert padding_is_zero(state[0]) and padding_is_zero(state[1])
    assert not np.array_equal(P, P0) and not np.array_equal(Q, Q0)


@pytest.mark.parametrize('adjust', [None, 'adagrad', 'rmsprop'])
@pytest.mark.parametrize('rank', [7, 10, 17, 40, 64])
@pytest.mark.parametrize('blocks', [1, 4, 32])
def test_one_epoch_is_bit_equal_to_the_restatement(hip_ops, blocks, rank, adjust):
    """the 300 x 150 fixture data with the kernels of kpmf_std (about 12 and 52 neighbours a row, three quarters of them across
    parts at B = 4): every lane-group width, B = 1 (all rows live), B = 4 and more than one workgroup (B = 32); P, Q, the
    snapshots and the state with leading dimensions of their own"""
    run_epochs(hip_ops, 'fixture', blocks, rank, adjust)


@pytest.mark.parametrize('adjust', [None, 'adagrad', 'rmsprop'])
def test_the_tiny_case_is_bit_equal_to_the_restatement(hip_ops, adjust):
    run_epochs(hip_ops, 'tiny', 4, 3, adjust)


@pytest.mark.parametrize('case, rank, adjust', [('tiny', 3, None), ('tiny', 3, 'adagrad'), ('tiny', 3, 'rmsprop'),
                                                ('fixture', 17, 'rmsprop')])
def test_half_identity_kernels_give_the_plain_sweep(hip_ops, case, rank, adjust):
    """both kernel matrices I / 2 (the diagonal stored, no off-diagonal entry): the kernelized term is (+0.0 + 0.5 * (p + p)) = p
    exactly, so kpmf_epoch leaves P, Q, the state and the squared error bit-equal to pmf_epoch on the same plan (B = 4), and
    the snapshots equal to P and Q"""
    ops = hip_ops
    u, i, v, n_users, n_items = case_of(case)[:5]
    plan = ops.kpmf_plan(device_csr(ops, u, i, v, n_users, n_items), 4, *half_identity_kernels(n_users, n_items))
    assert plan['ku_idx'].numel() == 0 and plan['ki_idx'].numel() == 0
    rng = np.random.RandomState(rank)
    P0, Q0 = rng.normal(scale=0.1, size=(n_users, rank)), rng.normal(scale=0.1, size=(n_items, rank))
    out = {}
    for kind in ('pmf', 'kpmf'):
        P, Q = ops.to_device(P0), ops.to_device(Q0)
        state = (ops.zeros(n_users, rank), ops.zeros(n_items, rank))
        if kind == 'kpmf':
            snaps = (ops.zeros(n_users, rank), ops.zeros(n_items, rank))
            sse = ops.kpmf_epoch(plan, P, Q, ETA, LAMBD, adjust=adjust, state=state if adjust else None, snapshots=snaps)
        else:
            sse = ops.pmf_epoch(plan, P, Q, ETA, LAMBD, adjust=adjust, state=state if adjust else None)
        out[kind] = [ops.to_host(x) for x in (P, Q) + state + (sse,)]
    for a, b in zip(out['pmf'], out['kpmf']):
        assert np.array_equal(a, b)
    assert np.array_equal(ops.to_host(snaps[0]), out['kpmf'][0]) and np.array_equal(ops.to_host(snaps[1]), out['kpmf'][1])
    assert not np.array_equal(out['kpmf'][0], P0) and not np.array_equal(out['kpmf'][1], Q0)
    assert bool(adjust) == bool(out['kpmf'][2].any())


def test_a_second_epoch_continues_from_the_first(hip_ops):
    """two epochs at B = 4: the first stratum of the second epoch reads — live and through the snapshots, which the caller's
    blocks keep between the calls — what the first epoch left"""
    run_epochs(hip_ops, 'fixture', 4, 10, 'rmsprop', epochs=2)
    run_epochs(hip_ops, 'fixture', 4, 10, None, epochs=2)


def test_epoch_checks_its_arguments(hip_ops):
    ops = hip_ops
    plan = device_plan(ops, 'tiny', 2)
    z = lambda *shape, **kw: ops.zeros(*shape, **kw)
    with pytest.raises(ValueError, match='rank'):
        ops.kpmf_epoch(plan, z(8, ref.MAX_RANK + 1), z(8, ref.MAX_RANK + 1), ETA, LAMBD)
    with pytest.raises(ValueError, match='block of shape'):
        ops.kpmf_epoch(plan, z(7, 3), z(8, 3), ETA, LAMBD)
    with pytest.raises(ValueError, match='block of shape'):
        ops.kpmf_epoch(plan, z(8, 3), z(8, 3), ETA, LAMBD, snapshots=(z(8, 3), z(8, 4)))
    with pytest.raises(ValueError, match='state'):
        ops.kpmf_epoch(plan, z(8, 3), z(8, 3), ETA, LAMBD, adjust='adagrad')
    with pytest.raises(ValueError, match='adjustment'):
        ops.kpmf_epoch(plan, z(8, 3), z(8, 3), ETA, LAMBD, adjust='adam')
    u, i, v, n_users, n_items, Ku, Ki = tiny_case()
    with pytest.raises(ValueError, match='plan of kpmf_plan'):
        ops.kpmf_epoch(ops.pmf_plan(device_csr(ops, u, i, v, n_users, n_items), 2), z(8, 3), z(8, 3), ETA, LAMBD)
    with pytest.raises(ValueError, match='kernel matrix of shape'):
        ops.kpmf_plan(device_csr(ops, u, i, v, n_users, n_items), 2, Ku[:7, :7], Ki)
    P = z(8, 3)
    with pytest.raises(RuntimeError, match='snapshot'):                 # the C entry: a snapshot that IS the block it copies
        ops.kpmf_epoch(plan, P, z(8, 3), ETA, LAMBD, snapshots=(P, z(8, 3)))


@pytest.mark.parametrize('name', FIXTURES)
def test_model_matches_the_reference(hip_ops, name):
    g = load_golden(name)
    m = ref.model_for(g, hip_ops)
    check_kpmf_model_against_fixture(m, g)
    P, Q, history = restated_solution(name)                                # and the restatement bit for bit
    assert np.array_equal(m.factors['userid'], P) and np.array_equal(m.factors['itemid'], Q)
    assert np.array_equal(np.array(m.rmse_history), history)


def test_two_identical_builds_give_identical_bits(hip_ops):
    g = load_golden('kpmf_rmsprop')
    runs = []
    for _ in range(2):
        m = ref.model_for(g, hip_ops)
        m.blocks = 16                                                      # a blocked, stale-neighbour epoch is deterministic too
        m.build(adjust_gradient='rmsprop')
        runs.append((m.factors['userid'].copy(), m.factors['itemid'].copy(), list(m.rmse_history), m.get_recommendations().copy()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
