"""LightFM (WARP), host side (no GPU): the schedule against BPR's, the blocks' disjointness with every drawn candidate, the NumPy
restatement (tests/lightfm_reference.py) against its own naive double, the draws' corner cases, the loss table, the package's
host functions, the two models on a CPU double of the device operators, and a learning test on a planted matrix with item
features and cold items."""
import functools

import numpy as np
import pytest

import bpr_reference as bref
import lightfm_reference as ref
from polara_amd import bpr, warp
from sweep_helpers import same_bits

# the learning test: planted_cold_start() (60 users, 40 warm + 8 cold items, 552 training positives, 8 labels), the restatement
LEARN = dict(rank=4, learning_rate=0.05, max_sampled=10, num_epochs=30, seed=7, blocks=3)
# the 8 x 8 corner case of the device tests: found with the restatement, see test_corner_case_has_its_properties
CORNER_SEED, CORNER_D, CORNER_RANK, CORNER_SCALE = 6, 3, 3, 40.0


@functools.lru_cache(maxsize=None)
def learned(featured=True):
    """(train, holdout, warm one-hot, cold likes, cold one-hot, the restated fit) on the planted matrix: computed once, shared
    with the device tests, never written to"""
    train, holdout, hot, cold_likes, cold_hot = ref.planted_cold_start()
    out = ref.fit(train, one_hot=hot if featured else None, **LEARN)
    for a in (train, holdout, hot, cold_likes, cold_hot) + tuple(out[k] for k in ('P', 'E', 'Q')):
        a.setflags(write=False)
    return train, holdout, hot, cold_likes, cold_hot, out


def corner_case():
    """(dense 8 x 8, one-hot 8 x 4, order, plan, candidates, (P0, E0, L0)) of the 8 x 8 case at B = 2: item 0 carries no label
    (a = 1, S = 0), label 0 is on every other item, label 1 on item 3 alone; the embeddings are scaled up so that margins hold"""
    rng = np.random.RandomState(CORNER_SEED)
    dense = (rng.rand(8, 8) < 0.4).astype(np.int8)
    hot = np.zeros((8, 4), dtype=np.int8)
    hot[1:, 0] = 1
    hot[3, 1] = 1
    hot[:, 2:] = rng.rand(8, 2) < 0.4
    hot[0] = 0
    order = ref.item_order(CORNER_SEED, 0, 8)
    plan = ref.make_plan(dense, 2, order)
    cand = ref.draw_candidates(plan, CORNER_SEED, 0, CORNER_D)
    init = tuple(CORNER_SCALE * x for x in ref.initial_embeddings(8, 8, 4, CORNER_RANK, CORNER_SEED))
    init[0][:, CORNER_RANK] = 1
    return dense, hot, order, plan, cand, init


# ---- the schedule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', [1, 2, 5])
def test_schedule_is_bprs_for_the_same_order(blocks):
    dense = ref.random_matrix()
    users, items = np.nonzero(dense)
    order = bpr.item_order(11, 3, 23)
    perm, block_ptr, item_part, item_ptr = bpr.block_schedule(users, items, 37, 23, blocks, order)
    for plan in (ref.make_plan(dense, blocks, order), bref.make_plan(dense, blocks, order)):
        assert np.array_equal(perm, plan['perm']) and np.array_equal(block_ptr, plan['block_ptr'])
        assert np.array_equal(item_part, plan['item_part']) and np.array_equal(item_ptr, plan['item_ptr'])


@pytest.mark.parametrize('blocks', [2, 5])
def test_blocks_of_a_stratum_share_no_row(blocks):
    """no two blocks of a stratum share a user, a positive item or ANY drawn candidate (violator or not)"""
    dense = ref.random_matrix()
    plan = ref.make_plan(dense, blocks, ref.item_order(3, 0, 23))
    cand = ref.draw_candidates(plan, 3, 0, 10)
    assert (cand >= 0).sum() > cand.size // 2
    B, bp = blocks, plan['block_ptr']
    for s in range(B):
        seen_users, seen_items = set(), set()
        for b in range(B):
            lo, hi = bp[s * B + b], bp[s * B + b + 1]
            users = set(plan['users'][lo:hi].tolist())
            drawn = cand[lo:hi]
            items = set(plan['items'][lo:hi].tolist()) | set(drawn[drawn >= 0].tolist())
            assert not (users & seen_users) and not (items & seen_items)
            seen_users |= users
            seen_items |= items


# ---- the draws -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', [1, 2, 5])
def test_candidates_stay_in_the_part_and_mark_seen_items(blocks):
    dense = ref.random_matrix()
    plan = ref.make_plan(dense, blocks, ref.item_order(5, 1, 23))
    cand = ref.draw_candidates(plan, 5, 1, 7)
    assert cand.shape == (plan['nnz'], 7) and cand.dtype == np.int32
    users = np.repeat(plan['users'][:, None], 7, axis=1)
    parts = np.repeat(plan['item_part'][plan['items']][:, None], 7, axis=1)
    ok = cand >= 0
    assert ok.any() and (~ok).any() and not dense[users[ok], cand[ok]].any()
    assert np.array_equal(plan['item_part'][cand[ok]], parts[ok])
    assert np.array_equal(cand[:, :3], ref.draw_candidates(plan, 5, 1, 3))        # the stream does not depend on D
    assert not np.array_equal(cand, ref.draw_candidates(plan, 5, 2, 7)) and not np.array_equal(cand, ref.draw_candidates(plan, 6, 1, 7))


@pytest.mark.parametrize('max_sampled', [1, 4])
def test_draw_corners(max_sampled):
    """a one-item part and a user who has seen a whole part give -1 throughout: the positive is quiet and nothing changes; D = 1"""
    dense, order = bref.corner_matrix()
    plan = ref.make_plan(dense, 2, order)
    assert np.array_equal(plan['item_ptr'], [0, 1, 6]) and plan['item_order'][0] == 0
    cand = ref.draw_candidates(plan, 5, 0, max_sampled)
    assert (cand[plan['items'] == 0] == -1).all() and (cand[plan['users'] == 0] == -1).all()
    rest = (plan['items'] != 0) & (plan['users'] != 0)
    assert rest.sum() == 2 and (cand[rest][:, 0] >= 1).all() and (cand[rest] != 0).all()
    P, E, _ = ref.initial_embeddings(8, 6, 0, 3, 1)
    P0, E0, AP, AE = P.copy(), E.copy(), np.ones_like(P), np.ones_like(E)
    got = ref.epoch(plan, cand, ref.loss_table(6, max_sampled), P, E, AP, AE, 0.05)
    assert got == (2, 13, 13 * max_sampled + 2)             # tiny scores: the first real candidate violates the margin
    touched_users, touched_items = plan['users'][rest], np.concatenate([plan['items'][rest], cand[rest][:, 0]])
    quiet_users = np.setdiff1d(np.arange(8), touched_users)
    quiet_items = np.setdiff1d(np.arange(6), touched_items)
    assert np.array_equal(P[quiet_users], P0[quiet_users]) and (AP[quiet_users] == 1).all()
    assert np.array_equal(E[quiet_items], E0[quiet_items]) and (AE[quiet_items] == 1).all()
    assert not np.array_equal(P[touched_users], P0[touched_users]) and (AE[touched_items] > 1).any()


def test_corner_case_has_its_properties():
    """the 8 x 8 case of the device tests: an item without labels, a label on one item, a label on every other item, a violator
    at the last draw, a quiet sample with real candidates, consecutive samples that share the user, and a pair of consecutive
    samples of one block that swap positive and violator (the forwarding case)"""
    dense, hot, order, plan, cand, (P, E, L) = corner_case()
    feat = ref.make_features(hot)
    assert feat['a'][0] == 1.0 and hot[:, 0].sum() == 7 and hot[:, 1].sum() == 1
    trace = []
    P, E, L = P.copy(), E.copy(), L.copy()
    counts = ref.epoch(plan, cand, ref.loss_table(8, CORNER_D), P, E, np.ones_like(P), np.ones_like(E), 0.05, feat, L, np.ones_like(L), trace)
    hits = dict(trace)
    assert counts[0] + counts[1] == plan['nnz'] and counts[0] > 0 and counts[1] > 0
    assert any(h == CORNER_D - 1 for h in hits.values())
    assert any(h < 0 and (cand[p] >= 0).any() for p, h in hits.items())
    bp, items, users = plan['block_ptr'], plan['items'], plan['users']
    swaps = shared = 0
    for k in range(len(bp) - 1):
        for p in range(bp[k], bp[k + 1] - 1):
            shared += users[p] == users[p + 1]
            if hits[p] >= 0 and hits[p + 1] >= 0:
                swaps += items[p + 1] == cand[p, hits[p]] and cand[p + 1, hits[p + 1]] == items[p]
    assert swaps >= 1 and shared >= 1


# ---- the loss table ------------------------------------------------------------------------------------------------------------
def test_loss_table():
    for n_items, D in ((40, 10), (8, 64), (10 ** 6, 64), (2, 3), (1, 2)):
        got, want = warp.loss_table(n_items, D), ref.loss_table(n_items, D)
        assert got.dtype == np.float64 and got.shape == (D,) and np.array_equal(got.view(np.int64), want.view(np.int64))
        floors = (n_items - 1) // np.arange(1, D + 1)
        assert (got[floors <= 1] == 0).all() and (got[floors > 1] > 0).all() and (got <= 10).all()
        assert (np.diff(got) <= 0).all()
    assert warp.loss_table(10 ** 6, 64)[0] == 10.0 and warp.loss_table(10 ** 6, 64)[63] == np.log(15624.0)
    assert warp.loss_table(40, 10)[0] == np.log(39.0) and warp.loss_table(8, 64)[3] == 0.0


# ---- the restatement against its naive double ---------------------------------------------------------------------------------
@pytest.mark.parametrize('blocks', [1, 3])
@pytest.mark.parametrize('featured', [False, True])
def test_restated_epoch_equals_the_naive_loop(featured, blocks):
    dense, hot = ref.random_matrix(), ref.random_features()
    rank, D = 5, 5
    init = [12.0 * x for x in ref.initial_embeddings(37, 23, hot.shape[1], rank, 2)]         # scores of order 1: margins hold
    init[0][:, rank] = 1
    a, b = [x.copy() for x in init], [x.copy() for x in init]
    sa, sb = [np.ones_like(x) for x in a], [np.ones_like(x) for x in b]
    feat = ref.make_features(hot) if featured else None
    for ep in range(2):
        order = ref.item_order(9, ep, 23)
        plan = ref.make_plan(dense, blocks, order)
        got = ref.epoch(plan, ref.draw_candidates(plan, 9, ep, D), ref.loss_table(23, D), a[0], a[1], sa[0], sa[1], 0.05, feat,
                        a[2] if featured else None, sa[2] if featured else None)
        want = ref.naive_epoch(dense, order, blocks, D, 9, ep, b[0], b[1], sb[0], sb[1], 0.05, hot if featured else None, b[2], sb[2])
        assert got == want and got[0] + got[1] == plan['nnz'] and got[0] > 0 and got[1] > 0 and got[2] > plan['nnz']
    for x, y in zip(a + sa, b + sb):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    assert (a[0][:, rank] == 1).all() and (sa[0][:, rank] == 1).all() and a[1][:, rank].any()
    assert featured == (not np.array_equal(a[2], init[2])) and featured == bool((sa[2] > 1).any())


# ---- the package's host functions ----------------------------------------------------------------------------------------------
def test_initial_embeddings_feature_weights_and_default_blocks():
    from scipy.sparse import csr_matrix
    got = warp.initial_embeddings(5, 4, 3, 2, seed=8)
    rng = np.random.RandomState(8)
    for x, n in zip(got, (5, 4, 3)):
        assert np.array_equal(x[:, :2], (rng.rand(n, 2) - 0.5) / 2)
    assert (got[0][:, 2] == 1).all() and (got[1][:, 2] == 0).all() and (got[2][:, 2] == 0).all()
    for x, y in zip(got, ref.initial_embeddings(5, 4, 3, 2, 8)):
        assert np.array_equal(x, y)
    assert warp.initial_embeddings(5, 4, 0, 2, seed=8)[2].shape == (0, 3)
    hot = ref.random_features()
    a, F = warp.feature_weights(csr_matrix(hot))
    feat = ref.make_features(hot)
    assert np.array_equal(a, feat['a']) and a[0] == 1.0 and np.array_equal(a, 1.0 / (1 + hot.sum(1)))
    assert np.array_equal(F.indptr, feat['row_ptr']) and np.array_equal(F.indices, feat['row_idx']) and np.array_equal(F.data, feat['row_val'])
    Fc = F.tocsc()
    Fc.sort_indices()
    assert np.array_equal(Fc.indptr, feat['col_ptr']) and np.array_equal(Fc.indices, feat['col_idx']) and np.array_equal(Fc.data, feat['col_val'])
    assert warp.default_blocks(20_000_000, 138_493, 26_744) == bpr.default_blocks(20_000_000, 138_493, 26_744)
    assert 'UNMEASURED' in warp.default_blocks.__doc__


def test_exports_and_defaults():
    import polara_amd
    from polara_amd.data import ArrayData
    assert {'LightFMWrapper', 'LightFMItemColdStart'} <= set(polara_amd.__all__)
    assert polara_amd.LightFMWrapper is warp.LightFMWrapper and polara_amd.LightFMItemColdStart is warp.LightFMItemColdStart
    users, items = np.nonzero(ref.random_matrix())
    data = ArrayData((users, items, np.ones(len(users))), n_users=37, n_items=23, fields=('userid', 'itemid', 'rating'))
    m = polara_amd.LightFMWrapper(data, ops=ref.numpy_ops())
    got = {k: getattr(m, k) for k in ('rank', 'loss', 'learning_schedule', 'learning_rate', 'max_sampled', 'seed', 'item_features',
                                      'item_identity', 'normalize_item_features', 'item_alpha', 'user_alpha', 'fit_params', 'fit_method',
                                      'user_features', 'blocks', 'reshuffle_items', 'method', 'warp_history')}
    assert got == dict(rank=10, loss='warp', learning_schedule='adagrad', learning_rate=0.05, max_sampled=10, seed=0, item_features=None,
                       item_identity=True, normalize_item_features=True, item_alpha=0.0, user_alpha=0.0, fit_params={}, fit_method='fit',
                       user_features=None, blocks=None, reshuffle_items=True, method='LightFM', warp_history=None)
    assert m.factors == {} and m.build_stats == {}


# ---- the models on a CPU double of the device operators ------------------------------------------------------------------------
def planted_model(ops, featured=True, cold=False, **settings):
    """LightFMWrapper / LightFMItemColdStart on the planted matrix with the public parameters of LEARN — shared with the device
    tests"""
    from scipy.sparse import csr_matrix
    from polara_amd.data import ArrayData, ItemColdStartArrayData
    train, holdout, hot, cold_likes, cold_hot = learned()[:5]
    users, items = np.nonzero(train)
    triplets = (users, items, np.ones(len(users)))
    if cold:
        fans, cold_items = np.nonzero(cold_likes)
        data = ItemColdStartArrayData(triplets, (fans, cold_items, np.ones(len(fans))), csr_matrix(hot), csr_matrix(cold_hot),
                                      n_users=train.shape[0], n_items=train.shape[1], fields=('userid', 'itemid', 'rating'))
        m = warp.LightFMItemColdStart(data, ops=ops)
    else:
        data = ArrayData(triplets, n_users=train.shape[0], n_items=train.shape[1],
                         holdout=(np.arange(train.shape[0]), holdout, np.ones(train.shape[0])), fields=('userid', 'itemid', 'rating'))
        m = warp.LightFMWrapper(data, item_features=csr_matrix(hot) if featured else None, ops=ops)
    m.verbose = False
    m.rank, m.learning_rate, m.max_sampled, m.seed = LEARN['rank'], LEARN['learning_rate'], LEARN['max_sampled'], LEARN['seed']
    m.fit_params, m.blocks, m.topk = dict(epochs=LEARN['num_epochs'], num_threads=4), LEARN['blocks'], 5
    for key, value in settings.items():
        setattr(m, key, value)
    return m


def check_model_against_the_restated_fit(m, featured=True):
    train, holdout, hot, cold_likes, cold_hot, out = learned(featured)
    m.build()
    assert m.method == 'LightFM' and set(m.factors) == {'userid', 'itemid', 'itemid_identity', 'itemid_features'}
    assert same_bits(m.factors['userid'], out['P']) and same_bits(m.factors['itemid'], out['Q'])
    assert same_bits(m.factors['itemid_identity'], out['E'])
    if featured:
        assert same_bits(m.factors['itemid_features'], out['L']) and not np.array_equal(out['Q'], out['E'])
    else:
        assert m.factors['itemid_features'].shape == (0, LEARN['rank'] + 1) and same_bits(out['Q'], out['E'])
    stats = m.build_stats
    assert tuple(m.warp_history) == tuple(out['history'])
    assert stats['trained'] == out['trained'] and stats['quiet'] == out['quiet'] and stats['draws'] == out['draws']
    assert len(m.iterations_time) == LEARN['num_epochs'] == stats['epochs'] and stats['blocks'] == LEARN['blocks']
    assert stats['candidate_bytes'] == int(train.sum()) * LEARN['max_sampled'] * 4 and stats['max_sampled'] == LEARN['max_sampled']
    assert stats['label_steps_per_epoch'] == (LEARN['blocks'] if featured else 0)
    assert all(t + q == int(train.sum()) for t, q in zip(stats['trained'], stats['quiet']))
    assert np.array_equal(m.get_recommendations(), ref.top_lists(out['P'] @ out['Q'].T, m.topk, train))


def check_cold_start_against_the_restated_fit(m):
    """the lists of every cold item against argsort of the restated scores; rows whose k-th and (k + 1)-th restated scores are
    equal are excluded (there is none on this fixture)"""
    train, holdout, hot, cold_likes, cold_hot, out = learned(True)
    m.build()
    assert m.method == 'LightFM(cs)' and same_bits(m.factors['itemid_features'], out['L']) and same_bits(m.factors['userid'], out['P'])
    scores = ref.cold_queries(cold_hot, out['L']) @ out['P'].T
    ranked = -np.sort(-scores, axis=1)
    clear = ranked[:, m.topk - 1] > ranked[:, m.topk]
    assert clear.all()
    got = m.get_recommendations()
    assert got.shape == (cold_hot.shape[0], m.topk)
    assert np.array_equal(got[clear], ref.top_lists(scores, m.topk, np.zeros_like(scores))[clear])
    dense = m.slice_recommendations()
    assert dense.shape == scores.shape and np.allclose(dense, scores, rtol=0, atol=1e-12)


def check_model_refusals(m, n_items=40):
    for name, bad, match in (('loss', 'bpr', "loss='bpr'"), ('learning_schedule', 'adadelta', "learning_schedule='adadelta'"),
                             ('user_features', {'x': [[1]] * 60}, 'user_features'), ('item_identity', False, 'item_identity=False'),
                             ('normalize_item_features', False, 'normalize_item_features=False'), ('item_alpha', 1e-4, 'item_alpha'),
                             ('user_alpha', 1e-4, 'user_alpha'), ('fit_method', 'fit_partial', "fit_method='fit_partial'"),
                             ('fit_params', dict(sample_weight=1), 'sample_weight')):
        good = getattr(m, name)
        setattr(m, name, bad)
        with pytest.raises(NotImplementedError, match=match):
            m.build()
        setattr(m, name, good)
        assert not m._is_ready
    for bad in (0, 65):
        m.max_sampled = bad
        with pytest.raises(ValueError, match='max_sampled %d' % bad):
            m.build()
    m.max_sampled = 3
    for bad in (0, 64):
        m.rank = bad
        with pytest.raises(ValueError, match='rank %d' % bad):
            m.build()
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
        with pytest.raises(NotImplementedError, match='warm start'):
            m.get_recommendations()
    finally:
        m.data.warm_start = False


@pytest.mark.parametrize('featured', [True, False])
def test_model_on_the_cpu_double(featured):
    check_model_against_the_restated_fit(planted_model(ref.numpy_ops(), featured), featured)


def test_cold_start_model_on_the_cpu_double():
    check_cold_start_against_the_restated_fit(planted_model(ref.numpy_ops(), cold=True))


def test_model_refusals_on_the_cpu_double():
    check_model_refusals(planted_model(ref.numpy_ops(), fit_params=dict(epochs=1)))

    class World2:
        world = 2
    with pytest.raises(NotImplementedError, match='multi-process'):
        warp.warp_fit(ref.numpy_ops(), None, 4, 0.05, 10, 1, comm=World2())
    from polara_amd.data import ArrayData
    users, items = np.nonzero(learned()[0])
    data = ArrayData((users, items, np.ones(len(users))), n_users=60, n_items=40, fields=('userid', 'itemid', 'rating'))
    with pytest.raises(ValueError, match='needs item features'):
        warp.LightFMItemColdStart(data, ops=ref.numpy_ops())


def test_a_dict_of_label_lists_is_encoded_with_stack_features():
    from polara_amd.coldstart import stack_features
    train, holdout, hot = learned()[:3]
    features = {'group': [[int(np.flatnonzero(row[:2])[0])] for row in hot], 'noise': [['n%d' % np.flatnonzero(row[2:])[0]] for row in hot]}
    one_hot, labels = stack_features(features)
    m = planted_model(ref.numpy_ops(), fit_params=dict(epochs=2), item_features=features)
    m.build()
    out = ref.fit(train, one_hot=one_hot.toarray(), **dict(LEARN, num_epochs=2))
    assert m.item_features_labels == labels and one_hot.shape == hot.shape
    assert same_bits(m.factors['itemid'], out['Q']) and same_bits(m.factors['itemid_features'], out['L'])


# ---- learning ----------------------------------------------------------------------------------------------------------------------
def test_the_restatement_learns_the_planted_structure():
    """B = 3, 30 epochs: held-out AUC 0.753 against 0.512 for ranking by item popularity; mean AUC of the cold items' user
    rankings 0.768 (chance 0.5); without features held-out AUC 0.744; warp_history (the quiet share) from 0.007 to 0.134"""
    train, holdout, hot, cold_likes, cold_hot, out = learned(True)
    plain = learned(False)[5]
    popularity = np.tile(train.sum(0).astype(np.float64), (train.shape[0], 1))
    auc, popular = ref.holdout_auc(out['P'] @ out['Q'].T, train, holdout), ref.holdout_auc(popularity, train, holdout)
    cold = ref.cold_auc(ref.cold_queries(cold_hot, out['L']) @ out['P'].T, cold_likes)
    print('held-out AUC: LightFM %.4f, popularity %.4f, without features %.4f; cold-start AUC %.4f; warp_history %.4f -> %.4f'
          % (auc, popular, ref.holdout_auc(plain['P'] @ plain['Q'].T, train, holdout), cold, out['history'][0], out['history'][-1]))
    assert auc >= popular + 0.15
    assert cold >= 0.65
    assert out['history'][-1] > out['history'][0]
    assert len(out['history']) == LEARN['num_epochs'] and (out['P'][:, LEARN['rank']] == 1).all()
