"""The factorisation model with side features (TCF) on the device: the plan and both feature dicts, one epoch of the sweep kernel
with its label launches (csrc/fm.hip), the label image and the label step alone against the NumPy restatement
(tests/fm_reference.py) BIT FOR BIT — parameters, step state, squared error, with the padding of every strided block untouched —
and the two models against the restated fit."""
import functools

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix

import fm_reference as ref
from polara_amd import fm  # noqa: F401  (the module under test: without it nothing here can run)
from sweep_helpers import MANY_STRATA_BLOCKS, device_csr, many_strata_matrix, padding_is_zero, same_bits, strided
from test_fm_host import (FACTOR_KEYS, LEARN, check_cold_start_against_the_restated_fit, check_model_against_the_restated_fit,
                          check_model_refusals, planted_model)

pytestmark = pytest.mark.gpu

REG, LIN_REG = 0.02, 0.03               # both non-zero and far from 1e-10: the count column of G matters
# (adjust, gamma, step): a label on every row sums a whole stratum's gradients, so plain SGD needs a small step to stay finite
RULES = dict(sgd=(None, 0.9, 0.002), adagrad=('adagrad', 0.9, 0.05), rmsprop=('rmsprop', 0.8, 0.05))
FEATURES = ('none', 'items', 'users', 'both')
RANKS = (1, 14, 15, 30, 31, 62)         # C = 3, 16 | 17, 32 | 33, 64: both sides of each width class
BLOCKS = (1, 2, 5)
PLAN_KEYS = ('perm', 'block_ptr', 'users', 'items', 'vals', 'row_nnz', 'col_nnz')


def ratings_csr(ops, ratings):
    users, items = np.nonzero(ratings)
    return ops.csr_from_coo(users.astype(np.int64), items.astype(np.int64), ratings[users, items].astype(np.float64), ratings.shape)


def corner_case():
    """(ratings 12 x 10, user one-hot 12 x 4, item one-hot 10 x 3) for B = 3 — see test_the_corner_case_is_bit_equal"""
    rng = np.random.RandomState(2)
    ratings = (rng.rand(12, 10) < 0.2) * rng.randint(1, 6, size=(12, 10)).astype(np.float64)
    ratings[:, 4] = np.where(np.arange(12) % 2 == 0, 3.0, ratings[:, 4])      # a popular item: consecutive samples share it
    ratings[11, :] = 0.0
    ratings[11, 9] = 2.0                                                       # a user with a single rating
    ratings[0:4, 5:] = 0.0                                                     # empties a block
    hot_u = np.zeros((12, 4), dtype=np.int8)
    hot_u[1:, 0] = 1                                                           # row 0 has no label; label 0 spans every part
    hot_u[1, 1] = hot_u[1, 2] = 1                                              # row 1 has three labels
    hot_u[7, 2] = 1                                                            # label 3 is on no row
    hot_i = np.zeros((10, 3), dtype=np.int8)
    hot_i[::2, 0] = 1
    hot_i[3:, 1] = 1
    return ratings, hot_u, hot_i


def corner_properties(plan, hot_u, width=16):
    """what the corner case must keep, from the host plan alone"""
    B, bp, users, items = plan['blocks'], plan['block_ptr'], plan['users'], plan['items']
    lengths = np.diff(bp)
    runs_of_one = same_item = False
    for x in range(B * B):
        u, i = users[bp[x]:bp[x + 1]], items[bp[x]:bp[x + 1]]
        if len(u) == 0:
            continue
        starts = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
        runs_of_one |= bool((np.diff(np.r_[starts, len(u)]) == 1).any())
        same_item |= bool(((i[1:] == i[:-1]) & (u[1:] != u[:-1])).any())
    shared = False
    for s in range(B):                                              # a label on rows of two different blocks of one stratum
        blocks_of = [set(np.flatnonzero(hot_u[users[bp[s * B + b]:bp[s * B + b + 1]]].any(0) if bp[s * B + b + 1] > bp[s * B + b]
                                        else np.zeros(hot_u.shape[1], dtype=bool))) for b in range(B)]
        shared |= any(blocks_of[x] & blocks_of[y] for x in range(B) for y in range(x + 1, B))
    return dict(run_of_one_user=runs_of_one, same_item_from_two_users=same_item, empty_block=bool((lengths == 0).any()),
                lane_group_past_B=B % (64 // width) != 0, row_without_label=bool((hot_u.sum(1) == 0).any()),
                label_without_row=bool((hot_u.sum(0) == 0).any()), row_with_three_labels=bool((hot_u.sum(1) == 3).any()),
                label_shared_by_two_blocks=shared)


def nontrivial_parameters(n_users, n_items, n_ul, n_il, rank, seed):
    """the seeded draw with biases and linear weights that are not zero"""
    P, E, LU, LI = ref.initial_parameters(n_users, n_items, n_ul, n_il, rank, seed)
    rng = np.random.RandomState(seed + 1)
    for X, c in ((P, rank), (E, rank + 1), (LU, rank), (LI, rank + 1)):
        X[:, c] = rng.normal(scale=0.2, size=len(X))
    return P, E, LU, LI


@functools.lru_cache(maxsize=None)
def restated_epoch(case, blocks, rank, features, rule, normalize=False, label_factors=True, epochs=1):
    """restated epochs: a dict computed once per case, never written to"""
    if case == 'corner':
        ratings, hot_u, hot_i = corner_case()
    elif case == 'many strata':
        ratings = many_strata_matrix() * np.random.RandomState(5).randint(1, 6, size=(300, 280)).astype(np.float64)
        hot_u, hot_i = np.zeros((300, 0), dtype=np.int8), np.zeros((280, 0), dtype=np.int8)
    elif case == 'no labels':
        ratings, hot_u, hot_i = ref.random_ratings(), np.zeros((37, 0), dtype=np.int8), np.zeros((23, 0), dtype=np.int8)
    else:
        ratings, hot_u, hot_i = ref.random_ratings(), ref.random_hot(37, 5, 1), ref.random_hot(23, 6, 2)
    with_u, with_i = features in ('users', 'both'), features in ('items', 'both')
    plan = ref.make_plan(ratings, blocks, hot_u if with_u else None, hot_i if with_i else None, normalize)
    mean = float(np.mean(ratings[np.nonzero(ratings)]))
    adjust, gamma, step = RULES[rule]
    init = nontrivial_parameters(ratings.shape[0], ratings.shape[1], hot_u.shape[1], hot_i.shape[1], rank, 1000 * blocks + rank)
    new = [x.copy() for x in init]
    state = [np.zeros_like(x) for x in init]
    sse = [ref.epoch(plan, mean, new[0], new[1], new[2] if with_u else None, new[3] if with_i else None, state if adjust else None,
                     step, REG, LIN_REG, adjust, gamma, label_factors) for _ in range(epochs)]
    out = dict(ratings=ratings, hot_u=hot_u, hot_i=hot_i, with_u=with_u, with_i=with_i, plan=plan, mean=mean, init=init,
               new=tuple(new), state=tuple(state), sse=sse)
    for a in (ratings, hot_u, hot_i) + tuple(init) + tuple(new) + tuple(state) + tuple(plan[k] for k in PLAN_KEYS):
        a.setflags(write=False)
    return out


def device_plan(ops, r, blocks, normalize=False):
    return ops.fm_plan(ratings_csr(ops, r['ratings']), blocks, csr_matrix(r['hot_u']) if r['with_u'] else None,
                       csr_matrix(r['hot_i']) if r['with_i'] else None, normalize)


def run_epoch(ops, case, blocks, rank, features, rule, normalize=False, label_factors=True, epochs=1):
    r = restated_epoch(case, blocks, rank, features, rule, normalize, label_factors, epochs)
    adjust, gamma, step = RULES[rule]
    plan = device_plan(ops, r, blocks, normalize)
    n_users, n_items = r['ratings'].shape
    C = rank + 2
    used = (True, True, r['with_u'], r['with_i'])
    pads = ((3, 1), (5, 2), (3, 2), (1, 0))
    dev = [strided(ops, x, *pad) if on else None for x, pad, on in zip(r['init'], pads, used)]
    state = [strided(ops, np.zeros_like(x), *pad) if on else None
             for x, pad, on in zip(r['init'], ((1, 1), (2, 0), (1, 0), (2, 2)), used)] if adjust else None
    junk = lambda n, cols, pad: strided(ops, np.full((n, cols), 7.0), *pad)       # whatever the buffers hold is overwritten
    work = (junk(n_users, C, (1, 1)) if r['with_u'] else None, junk(n_users, C + 1, (3, 1)) if r['with_u'] else None,
            junk(n_items, C, (2, 0)) if r['with_i'] else None, junk(n_items, C + 1, (1, 1)) if r['with_i'] else None)
    for want_sse in r['sse']:
        out = ops.fm_epoch(plan, r['mean'], dev[0], dev[1], dev[2], dev[3], state, step, REG, LIN_REG, adjust=adjust, gamma=gamma,
                           work=work, label_factors=label_factors)
        assert out.dtype == torch.float64 and tuple(out.shape) == (1,)
        assert float(out[0].item()) == want_sse
    for got, want, on in zip(dev + (state or []), r['new'] + (r['state'] if adjust else ()), used + (used if adjust else ())):
        if on:
            assert same_bits(ops.to_host(got), want) and padding_is_zero(got)
    for buffer, is_g in zip(work, (False, True, False, True)):
        if buffer is not None:
            assert padding_is_zero(buffer) and (not is_g or not bool(buffer.any()))
    assert not np.array_equal(r['new'][0], r['init'][0]) and not np.array_equal(r['new'][1], r['init'][1])
    k = rank
    assert (r['new'][0][:, k + 1] == 1).all() and (r['new'][1][:, k] == 1).all()      # the constants were never stepped
    if r['with_u'] and r['hot_u'].shape[1]:
        assert not np.array_equal(r['new'][2], r['init'][2]) and not r['new'][2][:, k + 1].any()
    if r['with_i'] and r['hot_i'].shape[1]:
        assert not np.array_equal(r['new'][3], r['init'][3]) and not r['new'][3][:, k].any()
    return r


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', BLOCKS)
def test_device_plan_and_both_feature_dicts_equal_the_restatement(hip_ops, blocks):
    ops = hip_ops
    for normalize in (False, True):
        r = restated_epoch('random', blocks, 7, 'both', 'sgd', normalize)
        dev = device_plan(ops, r, blocks, normalize)
        assert dev['blocks'] == blocks and dev['nnz'] == r['plan']['nnz'] and dev['shape'] == r['plan']['shape']
        for key in PLAN_KEYS:
            got = ops.to_host(dev[key])
            assert got.dtype == r['plan'][key].dtype and np.array_equal(got, r['plan'][key]), key
        for side in ('user', 'item'):
            want = r['plan']['features'][side]
            assert dev['features'][side]['n_labels'] == want['n_labels']
            for key in ref.FEATURE_KEYS:
                got = ops.to_host(dev['features'][side][key])
                assert got.dtype == want[key].dtype and np.array_equal(got, want[key]), (side, key)
            assert normalize == bool((want['a'] != 1).any())
    plain = ops.fm_plan(device_csr(ops, r['ratings'] != 0), blocks)               # (ones: the schedule ignores the values)
    assert np.array_equal(ops.to_host(plain['perm']), r['plan']['perm']) and (ops.to_host(plain['vals']) == 1).all()
    assert plain['features'] == dict(user=None, item=None)


# ---- the sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('features', FEATURES)
@pytest.mark.parametrize('rank', RANKS)
@pytest.mark.parametrize('blocks', BLOCKS)
def test_one_epoch_is_bit_equal_to_the_restatement(hip_ops, blocks, rank, features):
    """every B, every rank on both sides of a width class and every set of featured sides; the step rule runs through the three
    along a Latin square of the other three (every rule meets every value of each of them; the full product of rules and
    feature sets is the next test): a covering subset of the 216 cases"""
    rule = tuple(RULES)[(BLOCKS.index(blocks) + RANKS.index(rank) + FEATURES.index(features)) % 3]
    run_epoch(hip_ops, 'random', blocks, rank, features, rule)


@pytest.mark.parametrize('rule', tuple(RULES))
@pytest.mark.parametrize('features', FEATURES)
def test_every_step_rule_with_every_set_of_featured_sides(hip_ops, features, rule):
    """two epochs each: the step state is kept; B = 3 at width 32 leaves a lane group without a block"""
    run_epoch(hip_ops, 'random', 3, 15, features, rule, epochs=2)


@pytest.mark.parametrize('rule', tuple(RULES))
def test_normalised_weights_and_unfactorised_side_data(hip_ops, rule):
    run_epoch(hip_ops, 'random', 2, 7, 'both', rule, normalize=True)
    r = run_epoch(hip_ops, 'random', 2, 7, 'both', rule, label_factors=False)
    assert same_bits(r['new'][2][:, :7], r['init'][2][:, :7]) and same_bits(r['new'][3][:, :7], r['init'][3][:, :7])


@pytest.mark.parametrize('rule', tuple(RULES))
def test_the_corner_case_is_bit_equal(hip_ops, rule):
    """12 x 10 at B = 3, rank 3 (width 16: four lane groups per wave, the fourth has no block).  The plan is checked here, on
    the host: if it loses a property the test fails instead of passing for nothing."""
    ratings, hot_u, hot_i = corner_case()
    properties = corner_properties(ref.make_plan(ratings, 3), hot_u)
    assert all(properties.values()), properties
    run_epoch(hip_ops, 'corner', 3, 3, 'both', rule)


@pytest.mark.parametrize('features', ['items', 'both'])
def test_features_switched_on_without_any_label(hip_ops, features):
    """n_labels = 0: the images are zero, no label launch runs, the result is the featureless one"""
    r = run_epoch(hip_ops, 'no labels', 2, 5, features, 'adagrad')
    plain = restated_epoch('no labels', 2, 5, 'none', 'adagrad')
    assert same_bits(r['new'][0], plain['new'][0]) and same_bits(r['new'][1], plain['new'][1]) and r['sse'] == plain['sse']


def test_more_strata_than_the_error_reduction_has_threads(hip_ops):
    """B = 257: the reduction of the block sums strides the strata over 256 threads, so stratum 256 is its second trip; that
    stratum is not empty"""
    r = restated_epoch('many strata', MANY_STRATA_BLOCKS, 1, 'none', 'sgd')
    assert r['plan']['block_ptr'][256 * 257] < r['plan']['nnz']
    run_epoch(hip_ops, 'many strata', MANY_STRATA_BLOCKS, 1, 'none', 'sgd')


# ---- the label launches alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', ['user', 'item'])
def test_the_label_image_alone_is_bit_equal(hip_ops, side):
    ops = hip_ops
    r = restated_epoch('random', 2, 15, 'both', 'sgd', True)
    plan = device_plan(ops, r, 2, True)
    L = r['init'][2 if side == 'user' else 3]
    feat = r['plan']['features'][side]
    S = ops.fm_label_image(plan, side, strided(ops, L, 3, 1))
    assert same_bits(ops.to_host(S), ref.label_image(feat, L)) and not ops.to_host(S)[0].any()
    X = r['init'][0 if side == 'user' else 1]
    got = ops.fm_representation(plan, side, ops.to_device(X), ops.to_device(L))
    assert same_bits(ops.to_host(got), feat['a'][:, None] * X + ref.label_image(feat, L))


@pytest.mark.parametrize('label_factors', [True, False])
@pytest.mark.parametrize('rule', tuple(RULES))
@pytest.mark.parametrize('side', ['user', 'item'])
def test_the_label_step_alone_is_bit_equal(hip_ops, side, rule, label_factors):
    """G with counts: rows that were not sampled (count 0, so the last-but-one label of the user side takes no step), rows
    sampled several times"""
    ops = hip_ops
    rank = 7
    r = restated_epoch('random', 2, rank, 'both', 'sgd')
    plan = device_plan(ops, r, 2)
    adjust, gamma, step = RULES[rule]
    feat = r['plan']['features'][side]
    n, C = len(feat['a']), rank + 2
    rng = np.random.RandomState(4)
    G = rng.normal(size=(n, C + 1))
    G[:, C] = rng.randint(0, 4, size=n)
    lonely = feat['n_labels'] - 2
    G[r['hot_u' if side == 'user' else 'hot_i'][:, lonely] != 0, C] = 0.0
    G[G[:, C] == 0] = 0.0
    L = r['init'][2 if side == 'user' else 3].copy()
    SL = rng.rand(*L.shape)
    L0 = L.copy()
    Gd, Ld, SLd = strided(ops, G, 3, 1), strided(ops, L, 1, 0), strided(ops, SL, 2, 2)
    ops.fm_label_step(plan, side, Gd, Ld, SLd if adjust else None, step, REG, LIN_REG, adjust=adjust, gamma=gamma,
                      label_factors=label_factors)
    ref.label_step(feat, G, L, SL if adjust else None, side == 'item', step, REG, LIN_REG, adjust, gamma, label_factors)
    assert same_bits(ops.to_host(Ld), L) and same_bits(ops.to_host(SLd), SL) and not bool(Gd.any()) and not G.any()
    assert padding_is_zero(Gd) and padding_is_zero(Ld) and padding_is_zero(SLd)
    bias = rank + 1 if side == 'item' else rank
    assert not np.array_equal(L[:, bias], L0[:, bias]) and same_bits(L[lonely], L0[lonely]) and same_bits(L[-1], L0[-1])
    assert label_factors != same_bits(L[:, :rank], L0[:, :rank])


def test_operators_check_their_arguments(hip_ops):
    ops = hip_ops
    r = restated_epoch('random', 2, 7, 'both', 'sgd')
    A = ratings_csr(ops, r['ratings'])
    for bad in (0, 24):
        with pytest.raises(ValueError, match='blocks'):
            ops.fm_plan(A, bad)
    with pytest.raises(ValueError, match='features for 22 items'):
        ops.fm_plan(A, 2, None, csr_matrix(r['hot_i'][:22]))
    with pytest.raises(ValueError, match='features for 36 users'):
        ops.fm_plan(A, 2, csr_matrix(r['hot_u'][:36]))
    plan, featured = ops.fm_plan(A, 2), device_plan(ops, r, 2)
    assert ops.fm_max_rank() == ref.MAX_RANK == 62
    with pytest.raises(ValueError, match='rank 63'):
        ops.fm_epoch(plan, 3.0, ops.zeros(37, 65), ops.zeros(23, 65), None, None, None, 0.01, REG, LIN_REG)
    with pytest.raises(ValueError, match='block of shape'):
        ops.fm_epoch(plan, 3.0, ops.zeros(36, 5), ops.zeros(23, 5), None, None, None, 0.01, REG, LIN_REG)
    with pytest.raises(ValueError, match='state'):
        ops.fm_epoch(plan, 3.0, ops.zeros(37, 5), ops.zeros(23, 5), None, None, None, 0.01, REG, LIN_REG, adjust='adagrad')
    with pytest.raises(ValueError, match='adjustment'):
        ops.fm_epoch(plan, 3.0, ops.zeros(37, 5), ops.zeros(23, 5), None, None, None, 0.01, REG, LIN_REG, adjust='adam')
    with pytest.raises(ValueError, match='without user features'):
        ops.fm_epoch(plan, 3.0, ops.zeros(37, 5), ops.zeros(23, 5), ops.zeros(5, 5), None, None, 0.01, REG, LIN_REG)
    with pytest.raises(ValueError, match='need the label embeddings'):
        ops.fm_epoch(featured, 3.0, ops.zeros(37, 5), ops.zeros(23, 5), None, None, None, 0.01, REG, LIN_REG)
    with pytest.raises(ValueError, match='no item features'):
        ops.fm_label_step(plan, 'item', ops.zeros(23, 6), ops.zeros(6, 5), None, 0.01, REG, LIN_REG)
    with pytest.raises(ValueError, match='block of shape'):                       # G without its count column
        ops.fm_label_step(featured, 'item', ops.zeros(23, 5), ops.zeros(6, 5), None, 0.01, REG, LIN_REG)
    # the C entry refuses a rank above its bound with an error code, whatever the host layer checked
    P = ops.zeros(37, 70)
    side = [0] + [None] * 7 + [None, 0, None, 0, None, 0, None, 0]
    rc = ops.lib.pk_fm_epoch_f64(ops.stream(), 2, 63, plan['nnz'], 37, 23, plan['block_ptr'].data_ptr(), plan['users'].data_ptr(),
                                 plan['items'].data_ptr(), plan['vals'].data_ptr(), 3.0, P.data_ptr(), P.stride(0), P.data_ptr() + 8,
                                 P.stride(0), 0.01, REG, LIN_REG, 0, None, 0, None, 0, 0.9, 1e-6, 1, *side, *side,
                                 ops.empty(4).data_ptr(), ops.empty(1).data_ptr())
    assert rc == -1 and b'rank' in ops.lib.pk_last_error()            # PK_E_INVALID


# ---- the models -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('features', ['both', 'none'])
def test_model_equals_the_restated_fit(hip_ops, features):
    check_model_against_the_restated_fit(planted_model(hip_ops, features), features)


def test_cold_start_lists_equal_the_restated_scores(hip_ops):
    check_cold_start_against_the_restated_fit(planted_model(hip_ops, cold=True))


def test_two_identical_builds_give_identical_bits_and_another_seed_other_factors(hip_ops):
    runs = []
    for seed in (LEARN['seed'], LEARN['seed'], LEARN['seed'] + 1):
        m = planted_model(hip_ops, seed=seed, max_iterations=3)
        m.build()
        runs.append(tuple(m.factors[k] for k in FACTOR_KEYS) + (np.array(m.rmse_history), m.get_recommendations()))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    assert all(not np.array_equal(a, b) for a, b in zip(runs[0][:6], runs[2][:6]))


def test_model_refusals(hip_ops):
    check_model_refusals(planted_model(hip_ops, max_iterations=1))
