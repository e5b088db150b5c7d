"""BPR, host side (no GPU): the schedule with an item order (polara_amd/bpr.py: block_schedule) against PMF's, the NumPy
restatement (tests/bpr_reference.py) against its own naive double, the draws' corner cases, the restated sigmoid against
1 / (1 + exp(x)) in extended precision, and a learning test on a planted matrix."""
import functools

import numpy as np
import pytest

import bpr_reference as ref
from polara_amd import bpr, pmf

# The largest relative error of the restated sigmoid found on the two grids below against numpy.longdouble (80-bit, eps 1.1e-19):
# 2.98e-16 at the 4 001 points of linspace(-40, 40); at +-0, +-1e-300 it is 0, at +-700 at most 8.7e-18.  The test allows twice
# that, so that a slightly different grid does not trip it, and in any case less than 1e-13.
SIGMOID_MAX_REL_ERR = 2.98e-16
FORWARDING_SEED = 12            # found with the restatement: see test_forwarding_seed_has_the_property
# the learning test: planted_matrix() (60 x 40, 584 training positives), rank 4, 10 epochs at B = 3 with reshuffled parts
LEARN = dict(rank=4, learning_rate=0.1, regularization=0.01, num_epochs=10, seed=7, blocks=3)

GRID = np.linspace(-40, 40, 4001)
POINTS = np.array([0.0, -0.0, 1e-300, -1e-300, 700.0, -700.0, 800.0, -800.0, np.nan])


@functools.lru_cache(maxsize=None)
def learned():
    """(train, holdout, P, Q, auc_history, skipped) of the restatement on the planted matrix: computed once, shared with the
    device tests, never written to"""
    train, holdout = ref.planted_matrix()
    P, Q, auc, skipped = ref.fit(train, **LEARN)
    for a in (train, holdout, P, Q):
        a.setflags(write=False)
    return train, holdout, P, Q, tuple(auc), tuple(skipped)


# ---- the schedule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', [1, 2, 5, 23])
def test_schedule_with_the_identity_order_is_pmfs(blocks):
    dense = ref.random_matrix()
    users, items = np.nonzero(dense)
    want = pmf.block_schedule(users, items, 37, 23, blocks)
    for order in (None, np.arange(23)):
        perm, block_ptr, item_part, item_ptr = bpr.block_schedule(users, items, 37, 23, blocks, order)
        assert np.array_equal(perm, want[0]) and np.array_equal(block_ptr, want[1])
        assert np.array_equal(item_part, pmf._parts(np.bincount(items, minlength=23), blocks, len(users)))
        assert np.array_equal(item_ptr, np.searchsorted(item_part, np.arange(blocks + 1)))
    plan = ref.make_plan(dense, blocks)
    assert np.array_equal(plan['perm'], want[0]) and np.array_equal(plan['block_ptr'], want[1])


@pytest.mark.parametrize('blocks', [1, 2, 5])
def test_schedule_of_the_package_equals_the_restated_one(blocks):
    dense = ref.random_matrix()
    users, items = np.nonzero(dense)
    order = bpr.item_order(11, 3, 23)
    assert np.array_equal(order, ref.item_order(11, 3, 23)) and np.array_equal(np.sort(order), np.arange(23))
    assert not np.array_equal(order, np.arange(23)) and not np.array_equal(order, bpr.item_order(11, 4, 23))
    assert not np.array_equal(order, bpr.item_order(12, 3, 23))
    perm, block_ptr, item_part, item_ptr = bpr.block_schedule(users, items, 37, 23, blocks, order)
    plan = ref.make_plan(dense, blocks, order)
    assert np.array_equal(perm, plan['perm']) and np.array_equal(block_ptr, plan['block_ptr'])
    assert np.array_equal(item_part, plan['item_part']) and np.array_equal(item_ptr, plan['item_ptr'])
    for c in range(blocks):                                             # part c is a contiguous run of the order
        assert (item_part[order[item_ptr[c]:item_ptr[c + 1]]] == c).all()


def test_schedule_refuses_bad_block_counts():
    users, items = np.nonzero(ref.random_matrix())
    for bad in (0, 24):
        with pytest.raises(ValueError, match='blocks'):
            bpr.block_schedule(users, items, 37, 23, bad)


@pytest.mark.parametrize('blocks', [2, 5])
def test_blocks_of_a_stratum_share_no_row(blocks):
    """no two blocks of a stratum share a user, a positive item or a drawn negative"""
    dense = ref.random_matrix()
    plan = ref.make_plan(dense, blocks, ref.item_order(3, 0, 23))
    neg = ref.draw_negatives(plan, 3, 0)
    assert (neg >= 0).sum() > plan['nnz'] // 2
    B, bp = blocks, plan['block_ptr']
    for s in range(B):
        seen_users, seen_items = set(), set()
        for b in range(B):
            lo, hi = bp[s * B + b], bp[s * B + b + 1]
            users = set(plan['users'][lo:hi].tolist())
            items = set(plan['items'][lo:hi].tolist()) | set(neg[lo:hi][neg[lo:hi] >= 0].tolist())
            assert not (users & seen_users) and not (items & seen_items)
            seen_users |= users
            seen_items |= items


# ---- the draws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', [1, 2, 5])
def test_draws_never_return_a_seen_item_and_stay_in_the_part(blocks):
    dense = ref.random_matrix()
    plan = ref.make_plan(dense, blocks, ref.item_order(5, 1, 23))
    neg = ref.draw_negatives(plan, 5, 1)
    drawn = neg >= 0
    assert drawn.any() and not dense[plan['users'][drawn], neg[drawn]].any()
    assert np.array_equal(plan['item_part'][neg[drawn]], plan['item_part'][plan['items'][drawn]])
    assert not np.array_equal(neg, ref.draw_negatives(plan, 5, 2)) and not np.array_equal(neg, ref.draw_negatives(plan, 6, 1))


def test_draw_corners():
    """a one-item part skips everything; a user who has seen a whole part is skipped in it"""
    dense, order = ref.corner_matrix()
    plan = ref.make_plan(dense, 2, order)
    assert np.array_equal(plan['item_ptr'], [0, 1, 6]) and plan['item_order'][0] == 0
    neg = ref.draw_negatives(plan, 5, 0)
    assert (neg[plan['items'] == 0] == -1).all()
    assert (neg[plan['users'] == 0] == -1).all()
    rest = (plan['items'] != 0) & (plan['users'] != 0)
    assert rest.sum() == 2 and (neg[rest] >= 1).all()
    P, Q = ref.initial_factors(8, 6, 3, 1)
    assert ref.epoch(plan, neg, P, Q, 0.1, 0.01)[:2] == (2, 13)


def test_forwarding_seed_has_the_property():
    plan = ref.make_plan(ref.forwarding_matrix(), 1, ref.item_order(FORWARDING_SEED, 0, 3))
    neg = ref.draw_negatives(plan, FORWARDING_SEED, 0)
    assert np.array_equal(plan['users'], [0, 0, 1, 2, 3, 4]) and np.array_equal(plan['items'], [0, 1, 2, 0, 1, 1])
    assert (neg >= 0).all() and neg[0] == neg[1] == 2
    assert neg[2] == plan['items'][3] and neg[3] == plan['items'][2]    # each one's negative is the other's positive


# ---- the restatement against its naive double ---------------------------------------------------------------------------------
@pytest.mark.parametrize('rank', [1, 7, 16, 40])
def test_restatement_with_one_block_equals_the_naive_loop(rank):
    dense = ref.random_matrix()
    P0, Q0 = ref.initial_factors(37, 23, rank, 2)
    P, Q, Pn, Qn = P0.copy(), Q0.copy(), P0.copy(), Q0.copy()
    for ep in range(2):
        order = ref.item_order(9, ep, 23)
        plan = ref.make_plan(dense, 1, order)
        got = ref.epoch(plan, ref.draw_negatives(plan, 9, ep), P, Q, 0.05, 0.01)
        assert got == ref.naive_epoch(dense, order, Pn, Qn, 0.05, 0.01, 9, ep)
        assert got[0] + got[1] == plan['nnz'] and got[0] > 0
    assert np.array_equal(P, Pn) and np.array_equal(Q, Qn)
    assert (P[:, rank] == 1).all() and Q[:, rank].any() and not np.array_equal(P[:, :rank], P0[:, :rank])


# ---- the sigmoid ---------------------------------------------------------------------------------------------------------------
def test_sigmoid_against_extended_precision():
    assert np.finfo(np.longdouble).eps < 1e-18
    bound = 2 * SIGMOID_MAX_REL_ERR
    assert bound < 1e-13
    x = np.concatenate([GRID, POINTS[:6]])
    got = ref.sigmoid(x)
    want = 1 / (1 + np.exp(x.astype(np.longdouble)))
    err = float((np.abs(got.astype(np.longdouble) - want) / want).max())
    print('largest relative error of the sigmoid: %.3e' % err)
    assert err <= bound
    assert got[4000 + 1] == got[4000 + 2] == 0.5 and got[2000] == 0.5
    edge = ref.sigmoid(POINTS[6:])
    assert edge[0] == 0.0 and edge[1] == 1.0 and np.isnan(edge[2])
    assert float(ref.sigmoid(np.float64(1e300))) == 0.0 and float(ref.sigmoid(np.float64(-np.inf))) == 1.0


# ---- the package's host functions ----------------------------------------------------------------------------------------------
def test_initial_factors_and_default_blocks():
    P0, Q0 = bpr.initial_factors(5, 4, 3, seed=8)
    rng = np.random.RandomState(8)
    assert np.array_equal(P0[:, :3], (rng.rand(5, 3) - 0.5) / 3) and np.array_equal(Q0[:, :3], (rng.rand(4, 3) - 0.5) / 3)
    assert (P0[:, 3] == 1).all() and (Q0[:, 3] == 0).all()
    for a, b in zip((P0, Q0), ref.initial_factors(5, 4, 3, 8)):
        assert np.array_equal(a, b)
    assert bpr.default_blocks(20_000_000, 138_493, 26_744) == min(pmf.default_blocks(20_000_000, 138_493, 26_744), 26_744 // 64)
    assert bpr.default_blocks(584, 60, 40) == 1 and bpr.default_blocks(10 ** 9, 10 ** 6, 6400) == 100


def test_exports_and_defaults():
    import polara_amd
    from pmf_reference import PMFNumpyOps
    from polara_amd.data import ArrayData
    assert 'ImplicitBPR' in polara_amd.__all__ and polara_amd.ImplicitBPR is bpr.ImplicitBPR
    users, items = np.nonzero(ref.random_matrix())
    data = ArrayData((users, items, np.ones(len(users))), n_users=37, n_items=23, fields=('userid', 'itemid', 'rating'))
    m = polara_amd.ImplicitBPR(data, ops=PMFNumpyOps())
    got = {k: getattr(m, k) for k in ('rank', 'learning_rate', 'regularization', 'num_epochs', 'num_threads', 'random_state', 'seed',
                                      'method', 'show_progress', 'blocks', 'reshuffle_items', 'auc_history', 'iterations_time')}
    assert got == dict(rank=10, learning_rate=0.01, regularization=0.01, num_epochs=100, num_threads=0, random_state=None, seed=None,
                       method='BPRMF', show_progress=False, blocks=None, reshuffle_items=True, auc_history=None, iterations_time=None)
    assert m.factors == {} and m.build_stats == {}
    assert polara_amd.ImplicitBPR(data, seed=4, ops=PMFNumpyOps()).random_state == 4


# ---- the model on a CPU double of the device operators -----------------------------------------------------------------------------
def planted_model(ops, **settings):
    """ImplicitBPR on the planted matrix with the public parameters of LEARN — shared with the device tests"""
    from polara_amd.data import ArrayData
    train, holdout = learned()[:2]
    users, items = np.nonzero(train)
    data = ArrayData((users, items, np.ones(len(users))), n_users=train.shape[0], n_items=train.shape[1],
                     holdout=(np.arange(train.shape[0]), holdout, np.ones(train.shape[0])), fields=('userid', 'itemid', 'rating'))
    m = bpr.ImplicitBPR(data, seed=LEARN['seed'], ops=ops)
    m.verbose = False
    m.rank, m.learning_rate, m.regularization = LEARN['rank'], LEARN['learning_rate'], LEARN['regularization']
    m.num_epochs, m.blocks, m.topk = LEARN['num_epochs'], LEARN['blocks'], 5
    for key, value in settings.items():
        setattr(m, key, value)
    return m


def check_model_against_the_restated_fit(m):
    train, holdout, P, Q, auc, skipped = learned()
    m.build()
    assert m.method == 'BPRMF' and set(m.factors) == {'userid', 'itemid'}
    for got, want in ((m.factors['userid'], P), (m.factors['itemid'], Q)):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))
    assert tuple(m.auc_history) == auc and tuple(m.build_stats['skipped']) == skipped
    assert len(m.iterations_time) == LEARN['num_epochs'] == m.build_stats['epochs'] and m.build_stats['blocks'] == LEARN['blocks']
    assert all(t + s == int(train.sum()) for t, s in zip(m.build_stats['trained'], skipped))
    assert np.array_equal(m.get_recommendations(), ref.top_lists(P @ Q.T, m.topk, train))


def check_model_refusals(m, n_items=40):
    m.rank = 64
    with pytest.raises(ValueError, match='rank 64'):
        m.build()
    assert not m._is_ready
    m.rank = 4
    for bad in (0, n_items + 1):
        m.blocks = bad
        with pytest.raises(ValueError, match='blocks'):
            m.build()
    m.blocks = 2
    m.build()
    assert m._is_ready
    m.rank = 5                                                         # a rank change invalidates the model
    assert not m._is_ready
    m.build()
    assert m.factors['itemid'].shape == (n_items, 6)
    m.data.warm_start = True
    try:
        with pytest.raises(NotImplementedError, match='fold-in'):
            m.get_recommendations()
    finally:
        m.data.warm_start = False


def test_model_on_the_cpu_double():
    check_model_against_the_restated_fit(planted_model(ref.numpy_ops()))


def test_model_refusals_on_the_cpu_double():
    check_model_refusals(planted_model(ref.numpy_ops(), num_epochs=1))

    class World2:
        world = 2
    with pytest.raises(NotImplementedError, match='multi-process'):
        bpr.bpr_fit(ref.numpy_ops(), None, 4, 0.1, 0.01, 1, comm=World2())


# ---- learning ----------------------------------------------------------------------------------------------------------------------
def test_the_restatement_learns_the_planted_structure():
    """held-out AUC 0.847 against 0.507 for ranking by item popularity; auc_history from 0.531 to 0.851"""
    train, holdout, P, Q, auc, skipped = learned()
    popularity = np.tile(train.sum(0).astype(np.float64), (train.shape[0], 1))
    learned_auc, popular_auc = ref.holdout_auc(P @ Q.T, train, holdout), ref.holdout_auc(popularity, train, holdout)
    print('held-out AUC: BPR %.4f, popularity %.4f; auc_history %.4f -> %.4f' % (learned_auc, popular_auc, auc[0], auc[-1]))
    assert learned_auc > popular_auc
    assert auc[-1] > auc[0]
    assert len(auc) == len(skipped) == LEARN['num_epochs'] and (P[:, LEARN['rank']] == 1).all()
