"""LightFM (WARP) on the device: the plan, the feature matrices, the candidates, one epoch of the sweep kernel with its label
launches (csrc/warp.hip) and the label step alone against the NumPy restatement (tests/lightfm_reference.py) BIT FOR BIT, and
the two models against the restated fit."""
import functools

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import lightfm_reference as ref
from polara_amd import warp  # noqa: F401  (the module under test: without it nothing here can run)
from sweep_helpers import (MANY_STRATA_BLOCKS, MANY_STRATA_SEED, device_csr, many_strata_matrix, padding_is_zero, same_bits, strided,
                           trained_in_the_last_stratum)
from test_warp_host import (CORNER_D, CORNER_RANK, LEARN, check_cold_start_against_the_restated_fit,
                            check_model_against_the_restated_fit, check_model_refusals, corner_case, planted_model)

pytestmark = pytest.mark.gpu

LR = 0.05
PLAN_KEYS = ('perm', 'block_ptr', 'item_ptr', 'users', 'items', 'item_order', 'item_part')
FEATURE_KEYS = ('a', 'row_ptr', 'row_idx', 'row_val', 'col_ptr', 'col_idx', 'col_val')


def scaled_embeddings(n_users, n_items, n_labels, rank, seed):
    """the seeded draw, scaled so that scores are of order 1 and some candidates respect the margin; a bias that is not zero"""
    P, E, L = (5.0 * rank ** 0.75 * x for x in ref.initial_embeddings(n_users, n_items, n_labels, rank, seed))
    P[:, rank] = 1
    rng = np.random.RandomState(seed)
    E[:, rank] = rng.normal(scale=0.1, size=n_items)
    L[:, rank] = rng.normal(scale=0.1, size=n_labels)
    return P, E, L


@functools.lru_cache(maxsize=None)
def restated_epoch(case, blocks, rank, max_sampled, featured):
    """one restated epoch: a dict computed once per case, never written to"""
    if case == 'corner':
        dense, hot, order, plan, cand, init = corner_case()
        seed = None
    else:
        if case == 'many strata':
            dense, seed = many_strata_matrix(), MANY_STRATA_SEED
            hot = np.zeros((dense.shape[1], 0), dtype=np.int8)
        else:
            dense, hot = ref.random_matrix(), ref.random_features()
            seed = 1000 * blocks + 10 * rank + max_sampled
        order = ref.item_order(seed, 0, dense.shape[1])
        plan = ref.make_plan(dense, blocks, order)
        cand = ref.draw_candidates(plan, seed, 0, max_sampled)
        init = scaled_embeddings(dense.shape[0], dense.shape[1], hot.shape[1], rank, seed)
    feat = ref.make_features(hot) if featured else None
    table = ref.loss_table(dense.shape[1], max_sampled)
    new = [x.copy() for x in init]
    state = [np.ones_like(x) for x in init]
    trace = []
    counts = ref.epoch(plan, cand, table, new[0], new[1], state[0], state[1], LR, feat, new[2] if featured else None,
                       state[2] if featured else None, trace=trace)
    trained = np.zeros(plan['nnz'], dtype=bool)                           # per position of the schedule
    trained[[p for p, hit in trace if hit >= 0]] = True
    out = dict(dense=dense, hot=hot, order=order, seed=seed, plan=plan, cand=cand, table=table, init=init, new=tuple(new),
               state=tuple(state), counts=counts, feat=feat, trained=trained)
    for a in (dense, hot, order, cand, table) + tuple(init) + tuple(new) + tuple(state) + tuple(plan[k] for k in PLAN_KEYS):
        a.setflags(write=False)
    return out


def run_epoch(ops, case, blocks, rank, max_sampled, featured):
    r = restated_epoch(case, blocks, rank, max_sampled, featured)
    plan = ops.warp_plan(device_csr(ops, r['dense']), blocks, r['order'], csr_matrix(r['hot']) if featured else None)
    if r['seed'] is not None:
        cand = ops.warp_draw(plan, r['seed'], 0, max_sampled)
        assert np.array_equal(ops.to_host(cand), r['cand'])
    else:
        cand = ops.to_device(np.ascontiguousarray(r['cand']))
    n_items = r['dense'].shape[1]
    P, E = strided(ops, r['init'][0], 3, 1), strided(ops, r['init'][1], 5, 2)
    AP, AE = strided(ops, np.ones_like(r['init'][0]), 1, 1), strided(ops, np.ones_like(r['init'][1]), 2, 0)
    L = AL = work = None
    if featured:
        L, AL = strided(ops, r['init'][2], 3, 2), strided(ops, np.ones_like(r['init'][2]), 1, 0)
        work = (strided(ops, np.full((n_items, rank + 1), 7.0), 1, 1), strided(ops, np.full((n_items, rank + 1), 7.0), 3, 1))
    out = ops.warp_epoch(plan, cand, r['table'], P, E, (AP, AE, AL), LR, L, work=work)
    assert out.dtype == torch.int64 and tuple(out.shape) == (3,)
    assert tuple(int(c) for c in ops.to_host(out)) == r['counts']
    blocks_dev = (P, E, L, AP, AE, AL) if featured else (P, E, AP, AE)
    wanted = r['new'] + r['state'] if featured else r['new'][:2] + r['state'][:2]
    for got, want in zip(blocks_dev, wanted):
        assert same_bits(ops.to_host(got), want) and padding_is_zero(got)
    if featured:
        S, G = work
        assert not bool(G.any()) and padding_is_zero(G) and padding_is_zero(S)
    assert r['counts'][0] + r['counts'][1] == r['plan']['nnz']
    return r['counts']


# ---- plan, features and candidates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', [1, 2, 5])
def test_device_plan_features_and_candidates_equal_the_restatement(hip_ops, blocks):
    ops = hip_ops
    r = restated_epoch('random', blocks, 7, 10, True)
    dev = ops.warp_plan(device_csr(ops, r['dense']), blocks, r['order'], csr_matrix(r['hot']))
    assert dev['blocks'] == blocks and dev['nnz'] == r['plan']['nnz'] and dev['shape'] == r['plan']['shape']
    for key in PLAN_KEYS:
        got = ops.to_host(dev[key])
        assert got.dtype == r['plan'][key].dtype and np.array_equal(got, r['plan'][key]), key
    assert dev['features']['n_labels'] == r['feat']['n_labels']
    for key in FEATURE_KEYS:
        got = ops.to_host(dev['features'][key])
        assert got.dtype == r['feat'][key].dtype and np.array_equal(got, r['feat'][key]), key
    got = ops.to_host(ops.warp_draw(dev, r['seed'], 0, 10))
    assert got.dtype == np.int32 and got.shape == (r['plan']['nnz'], 10) and np.array_equal(got, r['cand'])
    assert (got >= 0).any() and (got < 0).any()
    assert ops.warp_plan(device_csr(ops, r['dense']), blocks, r['order'])['features'] is None


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_sampled', [1, 3, 10])
@pytest.mark.parametrize('rank', [1, 7, 15, 16, 31, 63])
@pytest.mark.parametrize('blocks', [1, 2, 5])
def test_one_epoch_without_features_is_bit_equal_to_the_restatement(hip_ops, blocks, rank, max_sampled):
    """k + 1 = 2, 8, 16 (lane groups of 16), 17, 32 (of 32), 64 (a full wave); one block per launch, fewer blocks than a wave
    holds and — at width 64 — more than one workgroup; one candidate, a partial batch and several batches; every block and its
    adagrad state with a leading dimension of its own"""
    counts = run_epoch(hip_ops, 'random', blocks, rank, max_sampled, False)
    assert counts[0] > 0 and counts[2] >= counts[0] + counts[1] * max_sampled


@pytest.mark.parametrize('rank', [7, 16, 63])
@pytest.mark.parametrize('blocks', [1, 4])
def test_one_epoch_with_features_is_bit_equal_to_the_restatement(hip_ops, blocks, rank):
    r = restated_epoch('random', blocks, rank, 5, True)
    if blocks > 1:                                                      # labels whose items fall in different parts
        parts = r['plan']['item_part']
        assert all(len(set(parts[np.flatnonzero(r['hot'][:, l])].tolist())) > 1 for l in range(3))
    counts = run_epoch(hip_ops, 'random', blocks, rank, 5, True)
    assert counts[0] > 0 and counts[1] > 0
    assert not np.array_equal(r['new'][2], r['init'][2]) and (r['state'][2] > 1).any()


def test_more_strata_than_the_counters_reduction_has_threads(hip_ops):
    """B = 257: the reduction of the block counters strides the strata over 256 threads, so stratum 256 is its second trip.  By
    the restatement alone a sample of that stratum is trained (a wrong trip would lose it) and some samples stay quiet."""
    r = restated_epoch('many strata', MANY_STRATA_BLOCKS, 1, 3, False)
    assert trained_in_the_last_stratum(r['plan'], r['trained']) and not r['trained'].all()
    trained, quiet, _ = run_epoch(hip_ops, 'many strata', MANY_STRATA_BLOCKS, 1, 3, False)
    assert trained > 0 and quiet > 0


def test_the_corner_case_is_bit_equal(hip_ops):
    """8 x 8 at B = 2 (tests/test_warp_host.py: test_corner_case_has_its_properties): an item without labels, a label on one
    item, a label on every other item, a violator at the last draw, a quiet sample, consecutive samples that share the user and
    a pair that swaps positive and violator"""
    counts = run_epoch(hip_ops, 'corner', 2, CORNER_RANK, CORNER_D, True)
    assert counts[0] > 0 and counts[1] > 0


@pytest.mark.parametrize('featured', [False, True])
def test_a_second_epoch_continues_from_the_first(hip_ops, featured):
    """two epochs on the device against two restated ones: the adagrad state is carried and the item order is new"""
    ops = hip_ops
    dense, hot, seed, B, D, rank = ref.random_matrix(), ref.random_features(), 21, 3, 4, 10
    feat = ref.make_features(hot) if featured else None
    A = device_csr(ops, dense)
    host = list(scaled_embeddings(37, 23, hot.shape[1], rank, seed))
    state = [np.ones_like(x) for x in host]
    dev = [ops.to_device(x) for x in host]
    dev_state = [ops.to_device(x) for x in state]
    table = ref.loss_table(23, D)
    for ep in range(2):
        order = ref.item_order(seed, ep, 23)
        plan_host = ref.make_plan(dense, B, order)
        want = ref.epoch(plan_host, ref.draw_candidates(plan_host, seed, ep, D), table, host[0], host[1], state[0], state[1], LR,
                         feat, host[2] if featured else None, state[2] if featured else None)
        plan = ops.warp_plan(A, B, order, csr_matrix(hot) if featured else None)
        got = ops.to_host(ops.warp_epoch(plan, ops.warp_draw(plan, seed, ep, D), table, dev[0], dev[1],
                                         (dev_state[0], dev_state[1], dev_state[2] if featured else None), LR,
                                         dev[2] if featured else None))
        assert tuple(int(c) for c in got) == want
    n = 3 if featured else 2
    for got, want in zip(dev[:n] + dev_state[:n], host[:n] + state[:n]):
        assert same_bits(ops.to_host(got), want)
    assert (state[0][:, :rank] > 1).any() and (state[0][:, rank] == 1).all()
    if featured:
        assert same_bits(ops.to_host(ops.warp_representation(plan, dev[1], dev[2])), ref.representation(host[1], feat, host[2]))
        assert same_bits(ops.to_host(ops.warp_label_image(plan, dev[2])), ref.label_image(feat, host[2]))


def test_the_label_step_alone_is_bit_equal(hip_ops):
    ops = hip_ops
    r = restated_epoch('random', 4, 7, 5, True)
    plan = ops.warp_plan(device_csr(ops, r['dense']), 4, r['order'], csr_matrix(r['hot']))
    rng = np.random.RandomState(4)
    G, L, AL = rng.normal(size=(23, 8)), r['init'][2].copy(), 1 + rng.rand(r['hot'].shape[1], 8)
    Gd, Ld, ALd = strided(ops, G, 3, 1), strided(ops, L, 1, 0), strided(ops, AL, 2, 2)
    ops.warp_label_step(plan, Gd, Ld, ALd, LR)
    ref.label_step(r['feat'], G, L, AL, LR)
    assert same_bits(ops.to_host(Ld), L) and same_bits(ops.to_host(ALd), AL) and not bool(Gd.any()) and not G.any()
    assert padding_is_zero(Gd) and padding_is_zero(Ld) and padding_is_zero(ALd)


def test_operators_check_their_arguments(hip_ops):
    ops = hip_ops
    dense, hot = ref.random_matrix(), ref.random_features()
    A = device_csr(ops, dense)
    for bad in (0, 24):
        with pytest.raises(ValueError, match='blocks'):
            ops.warp_plan(A, bad)
    with pytest.raises(ValueError, match='features for 22 items'):
        ops.warp_plan(A, 2, None, csr_matrix(hot[:22]))
    plan = ops.warp_plan(A, 2)
    for bad in (0, 65):
        with pytest.raises(ValueError, match='max_sampled'):
            ops.warp_draw(plan, 1, 0, bad)
    with pytest.raises(ValueError, match='32 unsigned bits'):
        ops.warp_draw(plan, 2 ** 32, 0, 3)
    cand, table = ops.warp_draw(plan, 1, 0, 3), ref.loss_table(23, 3)
    max_rank = ops.warp_max_rank()
    assert max_rank == ref.MAX_RANK == 63
    ones = lambda n, c: ops.to_device(np.ones((n, c)))
    with pytest.raises(ValueError, match='rank 64'):
        ops.warp_epoch(plan, cand, table, ops.zeros(37, 65), ops.zeros(23, 65), (ones(37, 65), ones(23, 65), None), LR)
    with pytest.raises(ValueError, match='block of shape'):
        ops.warp_epoch(plan, cand, table, ops.zeros(36, 4), ops.zeros(23, 4), (ones(36, 4), ones(23, 4), None), LR)
    with pytest.raises(ValueError, match='block of shape'):
        ops.warp_epoch(plan, cand, table, ops.zeros(37, 4), ops.zeros(23, 4), (ones(37, 4), ones(23, 5), None), LR)
    with pytest.raises(ValueError, match='candidates'):
        ops.warp_epoch(plan, cand[:-1], table, ops.zeros(37, 4), ops.zeros(23, 4), (ones(37, 4), ones(23, 4), None), LR)
    with pytest.raises(ValueError, match='loss table'):
        ops.warp_epoch(plan, cand, table[:2], ops.zeros(37, 4), ops.zeros(23, 4), (ones(37, 4), ones(23, 4), None), LR)
    with pytest.raises(ValueError, match='without item features'):
        ops.warp_epoch(plan, cand, table, ops.zeros(37, 4), ops.zeros(23, 4), (ones(37, 4), ones(23, 4), None), LR, ops.zeros(6, 4))
    featured = ops.warp_plan(A, 2, None, csr_matrix(hot))
    with pytest.raises(ValueError, match='need the label embeddings'):
        ops.warp_epoch(featured, cand, table, ops.zeros(37, 4), ops.zeros(23, 4), (ones(37, 4), ones(23, 4), None), LR)
    with pytest.raises(ValueError, match='no item features'):
        ops.warp_label_step(plan, ops.zeros(23, 4), ops.zeros(6, 4), ones(6, 4), LR)
    # the C entry refuses a rank above its bound with an error code, whatever the host layer checked
    P = ops.zeros(37, 66)
    rc = ops.lib.pk_warp_epoch_f64(ops.stream(), 2, 64, plan['nnz'], 23, 0, 3, plan['block_ptr'].data_ptr(), plan['users'].data_ptr(),
                                   plan['items'].data_ptr(), cand.data_ptr(), ops.to_device(table).data_ptr(), P.data_ptr(),
                                   P.stride(0), P.data_ptr() + 8, P.stride(0), P.data_ptr() + 16, P.stride(0), P.data_ptr() + 24,
                                   P.stride(0), LR, None, None, None, None, None, None, None, None, 0, None, 0, None, 0, None, 0,
                                   ops.empty(12).data_ptr(), ops.empty(3).data_ptr())
    assert rc == -1 and b'rank' in ops.lib.pk_last_error()            # PK_E_INVALID


# ---- the models -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('featured', [True, False])
def test_model_equals_the_restated_fit(hip_ops, featured):
    check_model_against_the_restated_fit(planted_model(hip_ops, featured), featured)


def test_cold_start_lists_equal_the_restated_scores(hip_ops):
    check_cold_start_against_the_restated_fit(planted_model(hip_ops, cold=True))


def test_two_identical_builds_give_identical_bits_and_another_seed_other_factors(hip_ops):
    runs = []
    for seed in (LEARN['seed'], LEARN['seed'], LEARN['seed'] + 1):
        m = planted_model(hip_ops, seed=seed, fit_params=dict(epochs=3))
        m.build()
        runs.append(tuple(m.factors[k] for k in ('userid', 'itemid', 'itemid_identity', 'itemid_features'))
                    + (np.array(m.warp_history), m.get_recommendations()))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    assert all(not np.array_equal(a, b) for a, b in zip(runs[0][:4], runs[2][:4]))


def test_model_refusals(hip_ops):
    check_model_refusals(planted_model(hip_ops, fit_params=dict(epochs=1)))
