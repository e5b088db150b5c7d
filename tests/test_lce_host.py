"""Local Collective Embeddings, host side (no GPU): the NumPy/SciPy restatement (tests/lce_reference.py) against the
reference's own fixtures (tests/golden/lce_*.npz from tests/golden/make_golden_lce.py), and both models' orchestration on
a CPU double of the device operators."""
import builtins
import sys

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import lce_reference as ref
from conftest import load_golden
from test_coldstart_host import EVAL_KEYS

FIXTURES = ['lce_std', 'lce_std_early', 'lce_cs', 'lce_cs_repr', 'lce_std_distance', 'lce_cs_rank7']
TOL = 1e-9              # of the largest entry: the `tol_scores` of test_coldstart_host.check_model_against_fixture


def close(a, b, tol=TOL):
    return a.shape == b.shape and np.abs(a - b).max() <= tol * np.abs(b).max()


def restated_scores_and_lists(g, W, HuT, HsT):
    topk = int(g['topk'])
    if bool(g['cold_start']):
        scores = ref.cold_scores(ref.coo(g, 'fc'), HsT, HuT)
        return scores, ref.top_lists(scores, topk)
    users = g['test_users']
    scores = HuT[users] @ W.T
    idx, shp = g['train_idx'], tuple(int(x) for x in g['train_shape'])
    train = sps.csr_matrix((g['train_val'], (idx[:, 0], idx[:, 1])), shape=shp)[users].tocoo()      # what the test users have seen
    return scores, ref.top_lists(scores, topk, seen=(train.row, train.col))


def check_solution(g, W, HuT, HsT, history):
    assert close(W, g['W']) and close(HuT, g['Hu'].T) and close(HsT, g['Hs'].T)
    assert len(history) == len(g['objective'])
    assert np.allclose(history, g['objective'], rtol=1e-9, atol=0)
    scores, lists = restated_scores_and_lists(g, W, HuT, HsT)
    n = g['scores'].shape[0]
    assert close(scores[:n], g['scores'])
    assert np.array_equal(lists, g['recs'])


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_matches_the_reference(name):
    g = load_golden(name)
    Xs, Xu, A, init, kw = ref.inputs(g)
    check_solution(g, *ref.solve(Xs, Xu, A, *init, **kw))
    assert float(g['min_rel_gap']) >= 1e-6 and float(g['cond_gram']) <= 1e6 and float(g['min_delta_ratio']) >= 1.01


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_with_the_users_permuted(name):
    """another summation order wherever a sum runs over users: the same factors, pass count and lists"""
    g = load_golden(name)
    Xs, Xu, A, init, kw = ref.inputs(g)
    perm = np.random.RandomState(3).permutation(Xu.shape[1])
    check_solution(g, *ref.solve(Xs, Xu, A, *init, user_perm=perm, **kw))


def test_the_fixtures_cover_what_was_asked():
    g = {n: load_golden(n) for n in FIXTURES}
    assert len(g['lce_std']['objective']) == 16 and int(g['lce_std']['max_iterations']) == 15
    assert 4 <= len(g['lce_std_early']['objective']) <= 10 and float(g['lce_std_early']['tolerance']) > 1.
    assert 'repr_users' in g['lce_cs_repr'] and len(g['lce_cs_repr']['repr_users']) == 100
    assert not bool(g['lce_std_distance']['binary_features']) and not np.all(g['lce_std_distance']['graph_val'] == 1.)
    assert int(g['lce_cs_rank7']['rank']) % 2 == 1
    for x in g.values():        # the graph: 1 + n_nbrs entries per row, the item itself among them
        n = int(x['graph_shape'][0])
        k = 1 + min(int(x['max_neighbours']), int(np.sqrt(n)))
        assert np.array_equal(np.bincount(x['graph_row'], minlength=n), np.full(n, k))


def check_lce_model_against_fixture(m, g, tol=TOL):
    """method name, factor keys and shapes, factors, scores, lists, evaluate() — shared with the device tests"""
    m.build()
    cold = bool(g['cold_start'])
    userid, itemid = m.data.fields.userid, m.data.fields.itemid
    assert m.method == str(g['model']) == ('LCE(cs)' if cold else 'LCE')
    assert set(m.factors) == {userid, itemid, f'{itemid}_features'} and itemid == 'item'
    assert close(m.factors[itemid], g['W'], tol) and close(m.factors[userid], g['Hu'].T, tol)
    assert close(m.factors[f'{itemid}_features'], g['Hs'].T, tol)
    assert m.build_stats['passes'] == len(g['objective'])
    assert np.allclose(m.build_stats['objective'], g['objective'], rtol=1e-9, atol=0)
    n = g['scores'].shape[0]
    if cold:
        assert m.filter_seen is False and m._prediction_key == 'item_cold' and m._prediction_target == 'userid'
        assert m.item_features_invgram.shape == (int(g['rank']),) * 2
        s = m.slice_recommendations(None, 0, n)
    else:
        test_data, shape, users = m._get_test_data()
        assert np.array_equal(users, g['test_users'])
        s, _ = m.slice_recommendations(test_data, shape, 0, n, users)
    assert close(s, g['scores'], tol)
    recs = m.get_recommendations()
    assert recs.dtype == np.int64 and np.array_equal(recs, g['recs'])
    scores = {type(x).__name__: x for x in m.evaluate('all')}
    for key in EVAL_KEYS:
        _, family, field = key.split('_', 2)
        assert np.isclose(getattr(scores[family], field), float(g[key]), rtol=1e-12, atol=0), key


@pytest.mark.parametrize('name', FIXTURES)
def test_models_on_the_cpu_double(name):
    g = load_golden(name)
    check_lce_model_against_fixture(ref.model_for(g, ref.LCENumpyOps()), g)


def test_exports_and_defaults():
    import polara_amd
    assert {'LCEModel', 'LCEModelItemColdStart'} <= set(polara_amd.__all__)
    m = polara_amd.LCEModel(ref.golden_data(load_golden('lce_std')), ops=ref.LCENumpyOps())
    got = {k: getattr(m, k) for k in ('rank', 'alpha', 'beta', 'max_neighbours', 'binary_features', 'seed', 'show_error',
                                      'regularization', 'max_iterations', 'tolerance')}
    assert got == dict(rank=10, alpha=0.1, beta=0.05, max_neighbours=10, binary_features=True, seed=None, show_error=False,
                       regularization=1, max_iterations=15, tolerance=1e-4)
    assert m.item_features is None and m.item_features_labels is None and m.method == 'LCE'
    with pytest.raises(ValueError, match='item features'):
        m.build()
    assert issubclass(polara_amd.LCEModelItemColdStart, polara_amd.LCEModel)


def test_a_rank_change_rebuilds():
    g = load_golden('lce_cs')
    m = ref.model_for(g, ref.LCENumpyOps())
    m.build()
    assert m._is_ready and len(m.training_time) == 1
    m.rank = 10
    assert m._is_ready                                    # the same rank: nothing happens
    m.rank = 6
    assert not m._is_ready and m._recommendations is None  # no truncation: LCE factors are not nested
    recs = m.recommendations
    assert len(m.training_time) == 2 and m.factors['userid'].shape[1] == 6 and recs.shape == g['recs'].shape
    assert m.item_features_invgram.shape == (6, 6)


def test_warm_start_raises():
    g = load_golden('lce_std')
    m = ref.model_for(g, ref.LCENumpyOps())
    m.build()
    m.data.warm_start = True
    with pytest.raises(NotImplementedError):
        m.get_recommendations()


def test_a_missing_graph_without_scikit_learn_raises(monkeypatch):
    g = load_golden('lce_std')
    m = ref.model_for(g, ref.LCENumpyOps())
    m.item_graph = None
    real_import = builtins.__import__

    def no_sklearn(name, *a, **kw):
        if name.split('.')[0] == 'sklearn':
            raise ImportError('hidden by the test')
        return real_import(name, *a, **kw)
    for mod in [k for k in sys.modules if k.split('.')[0] == 'sklearn']:
        monkeypatch.delitem(sys.modules, mod)
    monkeypatch.setattr(builtins, '__import__', no_sklearn)
    with pytest.raises(NotImplementedError, match='Install scikit-learn to construct graph for LCE model.'):
        m.build()


def test_the_graph_is_built_like_the_reference_when_none_is_given():
    pytest.importorskip('sklearn')
    g = load_golden('lce_std')
    m = ref.model_for(g, ref.LCENumpyOps())
    m.item_graph = None
    A = m._item_graph(ref.coo(g, 'ft'))
    n = A.shape[0]
    assert A.shape == tuple(g['graph_shape']) and np.array_equal(np.diff(A.indptr), np.full(n, 11)) and (A.data == 1).all()
    assert len(m.graph_time) == 1
    m.binary_features = False
    D = m._item_graph(ref.coo(g, 'ft'))
    assert D.shape == A.shape and not (D.data == 1).all()


def test_an_item_graph_of_the_wrong_shape_raises():
    g = load_golden('lce_std')
    m = ref.model_for(g, ref.LCENumpyOps())
    n = int(g['graph_shape'][0])
    for bad in (sps.identity(n - 1, format='csr'), sps.csr_matrix((n, n + 1)), np.eye(n)):
        m.item_graph = bad
        with pytest.raises(ValueError, match='item_graph'):
            m.build()


def test_seed_none_draws_from_the_global_generator():
    from polara_amd import lce
    np.random.seed(77)
    W, Hs, Hu = lce.initial_factors(5, 4, 3, 2, seed=None)
    rs = np.random.RandomState(77)
    assert np.array_equal(W, rs.rand(5, 2)) and np.array_equal(Hs, rs.rand(2, 4)) and np.array_equal(Hu, rs.rand(2, 3))
    rs = np.random.RandomState(9)
    W, Hs, Hu = lce.initial_factors(5, 4, 3, 2, seed=9)
    assert np.array_equal(W, rs.rand(5, 2)) and np.array_equal(Hs, rs.rand(2, 4)) and np.array_equal(Hu, rs.rand(2, 3))
    # through the model: two builds with seed None after the same global seed agree, and differ from another seed's
    g = load_golden('lce_cs')
    m = ref.model_for(g, ref.LCENumpyOps())
    m.seed = None
    np.random.seed(5)
    m.build()
    a = m.factors['item'].copy()
    np.random.seed(5)
    m.build()
    assert np.array_equal(a, m.factors['item'])
    m.build()
    assert not np.array_equal(a, m.factors['item'])


def test_init_overrides_the_draw_and_stats_are_filled():
    from polara_amd import lce
    g = load_golden('lce_std_early')
    Xs, Xu, A, init, kw = ref.inputs(g)
    stats = {}
    W, HuT, HsT = lce.local_collective_embeddings(ref.LCENumpyOps(), Xs, Xu, A, int(g['rank']), init=init, stats=stats, seed=12345, **kw)
    assert close(W.numpy(), g['W']) and close(HuT.numpy(), g['Hu'].T) and close(HsT.numpy(), g['Hs'].T)
    assert stats['passes'] == len(g['objective']) and np.allclose(stats['objective'], g['objective'], rtol=1e-9, atol=0)
    with pytest.raises(ValueError, match='initial factors'):
        lce.local_collective_embeddings(ref.LCENumpyOps(), Xs, Xu, A, int(g['rank']) + 1, init=init, **kw)
    with pytest.raises(ValueError, match='same items'):
        lce.local_collective_embeddings(ref.LCENumpyOps(), Xs, Xu[:-1], A, int(g['rank']), init=init, **kw)


def test_memory_guard_names_the_bytes():
    from polara_amd import lce
    need = lce.solver_bytes(20_000, 3_000, 138_000, 50, 60_000, 20_000_000, 220_000)
    assert need == 8 * 50 * 2 * (20_000 + 3_000 + 138_000) + 20 * (60_000 + 20_000_000) + 8 * 220_000
    assert lce.solver_bytes(10, 10, 100, 200, 0, 0, 0) == 8 * 200 * (2 * 120 + 100)       # the composed update's product block
    assert lce.check_solver_memory(20_000, 3_000, 138_000, 50, 60_000, 20_000_000, 220_000, 2 * need) == need
    with pytest.raises(MemoryError, match=str(need)):
        lce.check_solver_memory(20_000, 3_000, 138_000, 50, 60_000, 20_000_000, 220_000, 2 * need - 2)

    class Small(ref.LCENumpyOps):
        def free_bytes(self):
            return 1000
    g = load_golden('lce_std')
    with pytest.raises(MemoryError, match='bytes'):
        ref.model_for(g, Small()).build()


def test_multi_process_is_refused():
    from polara_amd import lce
    g = load_golden('lce_std')
    m = ref.model_for(g, ref.LCENumpyOps())

    class Two:
        world, rank = 2, 0
    m.comm = Two()
    with pytest.raises(NotImplementedError):
        m.build()
    Xs, Xu, A, init, kw = ref.inputs(g)
    with pytest.raises(NotImplementedError):
        lce.local_collective_embeddings(ref.LCENumpyOps(), Xs, Xu, A, 10, init=init, comm=Two(), **kw)


class CountingOps(ref.LCENumpyOps):
    def __init__(self):
        self.folds = 0

    def spmm(self, A, X, out=None, rows=None):
        self.folds += 1
        return super().spmm(A, X, out=out, rows=rows)


def test_recommend_without_queries_takes_the_old_path_and_with_them_skips_the_fold_in():
    from polara_amd import scoring
    rng = np.random.default_rng(4)
    n_users, n_items, K, topk = 70, 90, 6, 5
    V = torch.from_numpy(rng.random((n_items, K)))
    T = sps.random(n_users, n_items, density=0.1, random_state=5, format='csr')
    T.data[:] = 1.0
    ops = CountingOps()
    Td = ops.csr(T.indptr, T.indices, T.data, T.shape)
    image = scoring.FactorImage(ops, V)
    ops.folds = 0
    a = scoring.recommend(ops, image, Td, topk)
    folds = ops.folds
    b = scoring.recommend(ops, image, Td, topk, queries=None)
    assert folds >= 1 and ops.folds == 2 * folds and torch.equal(a, b)
    # the fold-in itself as queries: the same lists, and no fold-in product
    E = torch.from_numpy(np.asarray(T @ V.numpy()))
    ops.folds = 0
    c, s = scoring.recommend(ops, image, Td, topk, queries=E, return_scores=True)
    assert ops.folds == 0 and torch.equal(a, c)
    # other rows: brute force with the seen items pushed out
    Q = torch.from_numpy(rng.random((n_users, K)))
    got, sc = scoring.recommend(ops, image, Td, topk, queries=Q, return_scores=True)
    full = Q.numpy() @ V.numpy().T
    coo = T.tocoo()
    want = ref.top_lists(full, topk, seen=(coo.row, coo.col))
    assert np.array_equal(got.numpy(), want)
    assert np.allclose(sc.numpy(), np.take_along_axis(full, want, axis=1), rtol=1e-12)
    with pytest.raises(ValueError, match='queries'):
        scoring.recommend(ops, image, Td, topk, queries=Q[:-1])
    with pytest.raises(ValueError, match='queries'):
        scoring.recommend(ops, image, Td, topk, queries=Q.to(torch.float32))
