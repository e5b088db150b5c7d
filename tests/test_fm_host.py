"""The factorisation model with side features (TCF), host side (no GPU): the restated gradients against central differences of
the per-sample loss, the restatement at blocks = 1 against an independently written biased-MF SGD loop, a learning test on a
planted rating model with side features, and the models' surface on a CPU double of the device operators
(tests/fm_reference.py)."""
import functools

import numpy as np
import pytest

import fm_reference as ref
from polara_amd import fm, pmf
from sweep_helpers import same_bits

# the learning test and the models of the device tests: planted_ratings() (60 users, 40 warm + 8 cold items), the restatement
LEARN = dict(rank=4, num_epochs=15, seed=61, blocks=3, regularization=1e-3, linear_regularization=1e-3)


@functools.lru_cache(maxsize=None)
def learned(features='both', **changes):
    """(the planted data, the restated fit) — computed once per setting, shared with the device tests, never written to"""
    d = ref.planted_ratings()
    out = ref.fit(d['train'], hot_users=d['hot_users'] if features in ('both', 'users') else None,
                  hot_items=d['hot_items'] if features in ('both', 'items') else None, **dict(LEARN, **changes))
    for a in (d['train'], d['hot_users'], d['hot_items'], d['cold_hot'], out['P'], out['E'], out['Pt'], out['Qt']):
        a.setflags(write=False)
    return d, out


# ---- 1. the gradients ----------------------------------------------------------------------------------------------------------
def test_restated_gradients_equal_central_differences_of_the_loss():
    """Two samples (u1, i1), (u2, i2) whose users share user label 0 and whose items share item label 1; the loss is the sum
    of the two per-sample losses  (yhat - r)^2 / 2 + lambda_f / 2 |factor columns touched|^2 + lambda_lin / 2 |bias columns
    touched|^2, written here with np.dot from the definitions.  yhat is linear in any single parameter, so the loss is
    quadratic in it and the central difference with h = 2^-10 is exact up to the rounding of the two loss values: each is a
    sum of about a dozen rounded terms, so their difference carries at most about 16 eps max|loss|, divided by 2 h.  The
    tolerance is MULTIPLE = 16 times eps * max|loss| / h with the maximum taken over every loss value evaluated (printed)."""
    MULTIPLE, h, k = 16, 2.0 ** -10, 3
    C = k + 2
    rng = np.random.RandomState(0)
    hot_u = np.array([[1, 1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.int8)           # users 0 and 1 share label 0
    hot_i = np.array([[0, 1], [1, 1], [1, 0]], dtype=np.int8)                     # items 0 and 1 share label 1
    fu, fi = ref.make_features(hot_u, normalize=True), ref.make_features(hot_i, normalize=True)
    samples = ((0, 0, 4.0), (1, 1, 2.0))
    mean, reg, lin_reg = 3.0, 0.3, 0.7
    lam = ref.lambdas(k, reg, lin_reg)
    theta = dict(zip(('P', 'E', 'LU', 'LI'), ref.initial_parameters(3, 3, 3, 2, k, 5)))
    for name, bias_col in (('P', k), ('E', k + 1), ('LU', k), ('LI', k + 1)):
        theta[name][:, bias_col] = rng.normal(scale=0.5, size=len(theta[name]))
    Fu, Fi = fu['a'][:, None] * hot_u, fi['a'][:, None] * hot_i
    cols = dict(P=ref.stepped_columns(k, False), E=ref.stepped_columns(k, True), LU=ref.stepped_columns(k, False, True),
                LI=ref.stepped_columns(k, True, True))
    seen = []

    def loss(th):
        total = 0.0
        for u, i, r in samples:
            pt = fu['a'][u] * th['P'][u] + np.dot(Fu[u], th['LU'])
            qt = fi['a'][i] * th['E'][i] + np.dot(Fi[i], th['LI'])
            touched = [(th['P'][u], cols['P']), (th['E'][i], cols['E'])]
            touched += [(th['LU'][m], cols['LU']) for m in np.flatnonzero(hot_u[u])]
            touched += [(th['LI'][l], cols['LI']) for l in np.flatnonzero(hot_i[i])]
            total += 0.5 * (mean + np.dot(pt, qt) - r) ** 2 + sum(0.5 * np.dot(lam[c], x[c] ** 2) for x, c in touched)
        seen.append(total)
        return total

    # the restated gradients: the two samples from the same (unstepped) parameters, the labels from G as the label step does
    SU, SI = ref.label_image(fu, theta['LU']), ref.label_image(fi, theta['LI'])
    GU, GI = np.zeros((3, C + 1)), np.zeros((3, C + 1))
    grads = {name: np.zeros_like(x) for name, x in theta.items()}
    for u, i, r in samples:
        err, eq, ep, gp, gq = ref.sample(theta['P'][u], theta['E'][i], r, mean, ref.group_width(C), lam, fu['a'][u], SU[u], fi['a'][i], SI[i])
        grads['P'][u], grads['E'][i] = gp, gq
        GU[u, :C] += eq
        GU[u, C] += 1
        GI[i, :C] += ep
        GI[i, C] += 1
    for name, feat, G in (('LU', fu, GU), ('LI', fi, GI)):
        for l in range(feat['n_labels']):
            grads[name][l] = ref.label_gradient(feat, G, theta[name], l, lam)[0]
    assert ref.label_gradient(fu, GU, theta['LU'], 0, lam)[1] == 2.0              # the shared label counts both samples

    worst, checked = 0.0, 0
    quotients = []
    for name, x in theta.items():
        for r in range(x.shape[0]):
            for c in np.flatnonzero(cols[name]):
                plus, minus = ({n: v.copy() for n, v in theta.items()} for _ in range(2))
                plus[name][r, c] += h
                minus[name][r, c] -= h
                quotients.append(((loss(plus) - loss(minus)) / (2 * h), grads[name][r, c]))
                checked += 1
    tol = MULTIPLE * np.finfo(np.float64).eps * max(abs(v) for v in seen) / h
    worst = max(abs(a - b) for a, b in quotients)
    print('gradient check: %d parameters, max|loss| %.4f, tolerance %.3e, worst difference %.3e' % (checked, max(seen), tol, worst))
    assert checked == 2 * (k + 1) * 3 + (k + 1) * (3 + 2) and worst <= tol
    assert max(abs(b) for _, b in quotients) > 0.1                                # not a comparison of zeros
    # parameters no sample touches have a zero gradient on both sides: user 2, item 2, user label 2
    assert not grads['P'][2].any() and not grads['E'][2].any() and not grads['LU'][2].any()


# ---- 2. an independent loop at blocks = 1 ------------------------------------------------------------------------------------------
def biased_mf_sgd(ratings, mean, bu, bi, p, q, step, reg, lin_reg, epochs, reverse):
    """Biased matrix factorisation by SGD in row-major order of the ratings, written from the textbook: dense one-hot rows pick
    the parameters, np.dot sums.  `reverse` changes nothing but the order of the summations (the columns of the dot and the
    terms of the prediction).  Returns the RMSE history; the parameters are updated in place."""
    n_users, n_items = ratings.shape
    history = []
    for _ in range(epochs):
        sse, n = 0.0, 0
        for u in range(n_users):
            xu = np.zeros(n_users)
            xu[u] = 1.0
            for i in np.flatnonzero(ratings[u]):
                xi = np.zeros(n_items)
                xi[i] = 1.0
                pu, qi, b_u, b_i = np.dot(xu, p), np.dot(xi, q), np.dot(xu, bu), np.dot(xi, bi)
                if reverse:
                    pred = np.dot(pu[::-1], qi[::-1]) + b_i + b_u + mean
                else:
                    pred = mean + b_u + b_i + np.dot(pu, qi)
                err = pred - ratings[u, i]
                p[u] = pu - step * (err * qi + reg * pu)
                q[i] = qi - step * (err * pu + reg * qi)
                bu[u] = b_u - step * (err + lin_reg * b_u)
                bi[i] = b_i - step * (err + lin_reg * b_i)
                sse += err * err
                n += 1
        history.append(np.sqrt(sse / n))
    return history


def test_blocks_1_without_features_is_biased_mf_sgd():
    """solver='sgd', no features, blocks = 1: the restatement against the independent loop.  The tolerance is not fixed in
    advance: two copies of the loop that differ only in summation order are DIST apart (largest absolute difference over all
    parameters after the epochs); the restatement may be 4 x DIST from the loop, PMF's margin.  Measured here:
    DIST = 3.3e-16, restatement to loop 3.3e-16 (rank 8, 20 epochs, 255 ratings; both recorded in DESIGN 8q)."""
    ratings = ref.random_ratings()
    k, epochs, step, reg, lin_reg = 8, 20, 0.02, 0.02, 0.03
    mean = float(np.mean(ratings[np.nonzero(ratings)]))
    P0, E0, _, _ = ref.initial_parameters(37, 23, 0, 0, k, 3)
    rng = np.random.RandomState(4)
    P0[:, k], E0[:, k + 1] = rng.normal(scale=0.1, size=37), rng.normal(scale=0.1, size=23)
    copies = []
    for reverse in (False, True):
        bu, bi, p, q = P0[:, k].copy(), E0[:, k + 1].copy(), P0[:, :k].copy(), E0[:, :k].copy()
        history = biased_mf_sgd(ratings, mean, bu, bi, p, q, step, reg, lin_reg, epochs, reverse)
        copies.append((np.concatenate([p.ravel(), q.ravel(), bu, bi]), history))
    dist = np.abs(copies[0][0] - copies[1][0]).max()
    out = ref.fit(ratings, k, epochs, None, 1, regularization=reg, linear_regularization=lin_reg, solver='sgd', sgd_step_size=step,
                  init=(P0, E0, np.zeros((0, k + 2)), np.zeros((0, k + 2))), mean=mean)
    got = np.concatenate([out['P'][:, :k].ravel(), out['E'][:, :k].ravel(), out['P'][:, k], out['E'][:, k + 1]])
    gap = np.abs(got - copies[0][0]).max()
    print('independent loop: two summation orders %.3e apart, restatement to loop %.3e' % (dist, gap))
    assert dist > 0 and gap <= 4 * dist
    assert np.allclose(out['history'], copies[0][1], rtol=1e-12, atol=0) and out['history'][-1] < out['history'][0]
    assert (out['P'][:, k + 1] == 1).all() and (out['E'][:, k] == 1).all()      # the constants were never stepped
    assert np.abs(got - np.concatenate([P0[:, :k].ravel(), E0[:, :k].ravel(), P0[:, k], E0[:, k + 1]])).max() > 1e-3


# ---- 3. learning -------------------------------------------------------------------------------------------------------------------
def bias_baseline_rmse(train):
    """training RMSE of mu + user bias + item bias fitted by alternating means (20 rounds)"""
    mask = train != 0
    mu = train[mask].mean()
    bu, bi = np.zeros(train.shape[0]), np.zeros(train.shape[1])
    for _ in range(20):
        bu = np.where(mask.sum(1) > 0, ((train - mu - bi[None, :]) * mask).sum(1) / np.maximum(mask.sum(1), 1), 0.0)
        bi = np.where(mask.sum(0) > 0, ((train - mu - bu[:, None]) * mask).sum(0) / np.maximum(mask.sum(0), 1), 0.0)
    err = (train - mu - bu[:, None] - bi[None, :])[mask]
    return float(np.sqrt(np.mean(err * err)))


def holdout_rmse(d, out, users=None):
    u, i, r = d['holdout']
    keep = np.ones(len(u), dtype=bool) if users is None else np.isin(u, users)
    pred = out['mean'] + np.einsum('ij,ij->i', out['Pt'][u[keep]], out['Qt'][i[keep]])
    return float(np.sqrt(np.mean((pred - r[keep]) ** 2)))


def test_the_restatement_learns_the_planted_model():
    """B = 3, rank 4, 15 epochs, the default rule (rmsprop 0.9, step 0.05).  Observed: rmse_history 0.639 -> 0.206 after three
    epochs -> 0.150 at the end with both sides' features, against a training RMSE of 0.442 for mu + biases; on the holdout
    ratings of the 11 users with at most 8 training ratings 0.189 with features against 0.368 without (the printed line)."""
    d, out = learned('both')
    plain = learned('none')[1]
    history = out['history']
    baseline = bias_baseline_rmse(d['train'])
    few = np.flatnonzero((d['train'] != 0).sum(1) <= 8)
    with_f, without_f = holdout_rmse(d, out, few), holdout_rmse(d, plain, few)
    print('rmse_history %.4f -> %.4f -> %.4f; mu + biases %.4f; holdout of %d users with few ratings: %.4f with features, %.4f without'
          % (history[0], history[3], history[-1], baseline, len(few), with_f, without_f))
    assert len(history) == LEARN['num_epochs'] and history[1] < history[0] and history[2] < history[1] and history[3] < history[2]
    assert history[-1] < baseline
    assert len(few) >= 10 and with_f < without_f


# ---- 4. the surface ------------------------------------------------------------------------------------------------------------------
def planted_model(ops, features='both', cold=False, **settings):
    """TuriFactorizationRecommender / TuriFactorizationItemColdStart on the planted ratings with the public parameters of LEARN —
    shared with the device tests"""
    from scipy.sparse import csr_matrix
    from polara_amd.data import ArrayData, ItemColdStartArrayData
    d = learned()[0]
    train = d['train']
    users, items = np.nonzero(train)
    triplets = (users, items, train[users, items])
    side = dict(user_side_info=csr_matrix(d['hot_users']) if features in ('both', 'users') else None)
    if cold:
        data = ItemColdStartArrayData(triplets, d['cold'], csr_matrix(d['hot_items']), csr_matrix(d['cold_hot']),
                                      n_users=train.shape[0], n_items=train.shape[1], fields=('userid', 'itemid', 'rating'))
        m = fm.TuriFactorizationItemColdStart(data, ops=ops, **side)
    else:
        data = ArrayData(triplets, n_users=train.shape[0], n_items=train.shape[1], holdout=d['holdout'],
                         fields=('userid', 'itemid', 'rating'))
        m = fm.TuriFactorizationRecommender(data, ops=ops, item_side_info=csr_matrix(d['hot_items']) if features in ('both', 'items') else None,
                                            **side)
    m.verbose = False
    m.rank, m.max_iterations, m.seed, m.blocks, m.topk = LEARN['rank'], LEARN['num_epochs'], LEARN['seed'], LEARN['blocks'], 5
    m.regularization, m.linear_regularization = LEARN['regularization'], LEARN['linear_regularization']
    for key, value in settings.items():
        setattr(m, key, value)
    return m


FACTOR_KEYS = ('userid', 'itemid', 'itemid_identity', 'itemid_features', 'userid_identity', 'userid_features')


def check_model_against_the_restated_fit(m, features='both', **changes):
    d, out = learned(features, **changes)
    m.build()
    k = LEARN['rank']
    assert m.method == 'TCF' and set(m.factors) == set(FACTOR_KEYS)
    assert m.global_mean == out['mean'] == float(np.mean(d['train'][np.nonzero(d['train'])]))
    empty = np.zeros((0, k + 2))
    for key, want in zip(FACTOR_KEYS, (out['Pt'], out['Qt'], out['E'], out['LI'], out['P'], out['LU'])):
        assert same_bits(m.factors[key], empty if want is None else want), key
    epochs = changes.get('num_epochs', LEARN['num_epochs'])
    assert tuple(m.rmse_history) == tuple(out['history']) and len(m.iterations_time) == epochs
    stats = m.build_stats
    featured = dict(both=2, items=1, users=1, none=0)[features]
    assert stats['blocks'] == LEARN['blocks'] and stats['epochs'] == epochs
    assert stats['launches_per_epoch'] == LEARN['blocks'] * (1 + 2 * featured) + featured + 1
    assert stats['label_steps_per_epoch'] == (LEARN['blocks'] if featured else 0)
    scores = out['Pt'] @ out['Qt'].T
    assert np.array_equal(m.get_recommendations(), ref.top_lists(scores[d['holdout'][0]], m.topk, d['train'][d['holdout'][0]]))
    u, i, r = d['holdout']
    want = np.sqrt(np.mean((out['mean'] + np.einsum('ij,ij->i', out['Pt'][u], out['Qt'][i]) - r) ** 2))
    assert abs(m.evaluate_rmse() - want) <= 1e-12
    return out


def check_cold_start_against_the_restated_fit(m, normalize=False):
    """the lists of every cold item against a NumPy top-k of the restated scores (F_cold LI + w e_k) Pt^T; rows with an exact tie
    at the k-th place are excluded — their share is asserted to be 0 on this fixture"""
    d, out = learned('both', normalize=normalize) if normalize else learned('both')
    m.build()
    assert m.method == 'TCF(cs)' and same_bits(m.factors['itemid_features'], out['LI']) and same_bits(m.factors['userid'], out['Pt'])
    queries = ref.cold_queries(d['cold_hot'], out['LI'], normalize)
    assert (queries[:, LEARN['rank']] > 0).all()                                 # the constant: the user bias counts
    scores = queries @ out['Pt'].T
    ranked = -np.sort(-scores, axis=1)
    clear = ranked[:, m.topk - 1] > ranked[:, m.topk]
    assert (~clear).mean() == 0.0
    got = m.get_recommendations()
    assert got.shape == (d['cold_hot'].shape[0], m.topk)
    assert np.array_equal(got[clear], ref.top_lists(scores, m.topk, np.zeros_like(scores))[clear])
    dense = m.slice_recommendations()
    assert dense.shape == scores.shape and np.allclose(dense, scores, rtol=0, atol=1e-12)


def check_model_refusals(m, n_items=40):
    for name, bad, match in (('ranking_optimization', True, 'ranking_optimization=True'),
                             ('with_data_feedback', False, 'with_data_feedback=False'), ('binary_target', True, 'binary_target=True'),
                             ('solver', 'als', "solver='als'"), ('solver', 'lbfgs', "solver='lbfgs'"),
                             ('other_tc_params', dict(nmf=True), 'other_tc_params')):
        good = getattr(m, name)
        setattr(m, name, bad)
        with pytest.raises(NotImplementedError, match=match):
            m.build()
        setattr(m, name, good)
        assert not m._is_ready
    for bad in (0.0, 1.0, 1.5):
        m.adagrad_momentum_weighting = bad
        with pytest.raises(ValueError, match='adagrad_momentum_weighting'):
            m.build()
    m.adagrad_momentum_weighting = 0.9
    for bad in (0, 63):
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
    m.num_factors = 5                                                  # a rank change (by its alias) invalidates the model
    assert not m._is_ready and m.rank == 5
    m.build()
    assert m.factors['itemid'].shape == (n_items, 7)
    m.data.warm_start = True
    try:
        with pytest.raises(NotImplementedError, match='warm start'):
            m.get_recommendations()
        with pytest.raises(NotImplementedError, match='warm start'):
            m.evaluate_rmse()
    finally:
        m.data.warm_start = False


def test_exports_and_defaults():
    import polara_amd
    from polara_amd.data import ArrayData
    assert {'TuriFactorizationRecommender', 'TuriFactorizationItemColdStart'} <= set(polara_amd.__all__)
    assert polara_amd.TuriFactorizationRecommender is fm.TuriFactorizationRecommender
    assert polara_amd.TuriFactorizationItemColdStart is fm.TuriFactorizationItemColdStart
    assert not hasattr(polara_amd, 'KernelizedPMF') and not hasattr(polara_amd, 'RandomModel')
    ratings = ref.random_ratings()
    users, items = np.nonzero(ratings)
    data = ArrayData((users, items, ratings[users, items]), n_users=37, n_items=23, fields=('userid', 'itemid', 'rating'))
    m = polara_amd.TuriFactorizationRecommender(data, ops=ref.numpy_ops())
    names = ('method', 'rank', 'num_factors', 'seed', 'binary_target', 'solver', 'max_iterations', 'regularization', 'linear_regularization',
             'adagrad_momentum_weighting', 'sgd_step_size', 'side_data_factorization', 'ranking_optimization', 'ranking_regularization',
             'unobserved_rating_value', 'num_sampled_negative_examples', 'with_data_feedback', 'other_tc_params', 'item_side_info',
             'user_side_info', 'blocks', 'normalize_side_features', 'rmse_history', 'iterations_time', 'build_stats', 'global_mean')
    assert {k: getattr(m, k) for k in names} == dict(
        method='TCF', rank=10, num_factors=10, seed=61, binary_target=False, solver='auto', max_iterations=25, regularization=1e-10,
        linear_regularization=1e-10, adagrad_momentum_weighting=0.9, sgd_step_size=0, side_data_factorization=True,
        ranking_optimization=False, ranking_regularization=0.25, unobserved_rating_value=None, num_sampled_negative_examples=4,
        with_data_feedback=True, other_tc_params={}, item_side_info=None, user_side_info=None, blocks=None, normalize_side_features=False,
        rmse_history=None, iterations_time=None, build_stats={}, global_mean=None)
    assert m.factors == {}


def test_step_rules_initial_parameters_and_default_blocks():
    assert fm.step_rule('auto', 0.9, 0) == ('rmsprop', 0.9, 0.05) and fm.step_rule('adagrad', 0.5, 0.1) == ('rmsprop', 0.5, 0.1)
    assert fm.step_rule('adagrad', None, 0) == ('adagrad', pmf.RMSPROP_GAMMA, 0.05) and fm.step_rule('sgd', 0.9, 0) == (None, 0.9, 0.005)
    for args in (('auto', 0.9, 0), ('adagrad', None, 0.2), ('sgd', 0.9, 0)):
        assert fm.step_rule(*args) == ref.step_rule(*args)
    got = fm.initial_parameters(5, 4, 3, 2, 2, seed=8)
    rng = np.random.RandomState(8)
    for x, n in zip(got, (5, 4, 3, 2)):
        assert x.shape == (n, 4) and np.array_equal(x[:, :2], rng.normal(scale=0.1, size=(n, 2)))
    assert (got[0][:, 2] == 0).all() and (got[0][:, 3] == 1).all() and (got[1][:, 2] == 1).all() and (got[1][:, 3] == 0).all()
    assert not got[2][:, 2:].any() and not got[3][:, 2:].any()
    for x, y in zip(got, ref.initial_parameters(5, 4, 3, 2, 2, 8)):
        assert np.array_equal(x, y)
    assert fm.default_blocks(20_000_000, 138_493, 26_744) == pmf.default_blocks(20_000_000, 138_493, 26_744)
    assert 'UNMEASURED' in fm.default_blocks.__doc__
    from scipy.sparse import csr_matrix
    hot = ref.random_hot(23, 6, 2)
    for normalize in (False, True):
        a, F = fm.side_features(csr_matrix(hot), normalize)
        feat = ref.make_features(hot, normalize)
        assert np.array_equal(a, feat['a']) and np.array_equal(F.indptr, feat['row_ptr']) and np.array_equal(F.indices, feat['row_idx'])
        assert np.array_equal(F.data, feat['row_val']) and (a[0] == 1.0) and (normalize or (a == 1).all())


@pytest.mark.parametrize('features', ['both', 'items', 'users', 'none'])
def test_model_on_the_cpu_double(features):
    check_model_against_the_restated_fit(planted_model(ref.numpy_ops(), features), features)


def test_cold_start_model_on_the_cpu_double():
    check_cold_start_against_the_restated_fit(planted_model(ref.numpy_ops(), cold=True))


def test_normalised_cold_start_model_on_the_cpu_double():
    check_cold_start_against_the_restated_fit(planted_model(ref.numpy_ops(), cold=True, normalize_side_features=True), normalize=True)


def test_side_data_factorization_off_leaves_the_label_factors_zero():
    """the label rows keep exact zeros in their factor columns and only their linear weights move; P and E are drawn as ever"""
    out = check_model_against_the_restated_fit(planted_model(ref.numpy_ops(), side_data_factorization=False, max_iterations=3), 'both',
                                               label_factors=False, num_epochs=3)
    k = LEARN['rank']
    assert not out['LU'][:, :k].any() and not out['LI'][:, :k].any()
    assert out['LU'][:, k].any() and out['LI'][:, k + 1].any() and not out['LU'][:, k + 1].any() and not out['LI'][:, k].any()
    assert same_bits(out['Pt'][:, :k], out['P'][:, :k]) and not same_bits(out['Pt'][:, k], out['P'][:, k])


def test_model_refusals_on_the_cpu_double():
    check_model_refusals(planted_model(ref.numpy_ops(), max_iterations=1))

    class World2:
        world = 2
    with pytest.raises(NotImplementedError, match='multi-process'):
        fm.fm_fit(ref.numpy_ops(), None, 4, 1, 3.0, comm=World2())
    from polara_amd.data import ArrayData
    train = learned()[0]['train']
    users, items = np.nonzero(train)
    data = ArrayData((users, items, train[users, items]), n_users=60, n_items=40, fields=('userid', 'itemid', 'rating'))
    with pytest.raises(ValueError, match='needs item side information'):
        fm.TuriFactorizationItemColdStart(data, ops=ref.numpy_ops())


def test_a_dict_of_label_lists_is_encoded_with_stack_features():
    from polara_amd.coldstart import stack_features
    d = learned()[0]
    item_info = {'genre': [['g%d' % l for l in np.flatnonzero(row)] for row in d['hot_items']]}
    user_info = {'group': [['u%d' % l for l in np.flatnonzero(row)] for row in d['hot_users']]}
    hot_i, item_labels = stack_features(item_info)
    hot_u, user_labels = stack_features(user_info)
    m = planted_model(ref.numpy_ops(), max_iterations=2, item_side_info=item_info, user_side_info=user_info)
    m.build()
    out = ref.fit(d['train'], hot_users=hot_u.toarray(), hot_items=hot_i.toarray(), **dict(LEARN, num_epochs=2))
    assert m.item_features_labels == item_labels and m.user_features_labels == user_labels
    assert same_bits(m.factors['itemid'], out['Qt']) and same_bits(m.factors['userid_features'], out['LU'])
