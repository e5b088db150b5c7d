"""Local Collective Embeddings on the device: the update and reduction kernels (csrc/lce.hip) against NumPy, the solver
against the reference's fixtures (tests/golden/lce_*.npz), `scoring.recommend(queries=...)` against brute-force fp64, both
models against the fixtures, and one planted case at scale against the restatement (tests/lce_reference.py)."""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

import lce_reference as ref
from conftest import load_golden
from i2i_reference import select, tie_aware_mismatches
from recorded_calls import sweeps
from sweep_helpers import padding_is_zero, strided
from test_lce_host import FIXTURES, TOL, check_lce_model_against_fixture, close

pytestmark = pytest.mark.gpu

TIE_TOL = 1e-12                     # as in test_gpu_coldstart.py: O(1) sums of <= 100 fp64 products


def launches(rec):
    """names of the recorded library calls that enqueue work (first argument: the stream), as tools/bench_coldstart.py counts
    them; planning queries (work sizes, the fused bound) are host functions"""
    return [n for n, f, a in rec.calls if a and hasattr(a[0], 'value')]


def update_case(rng, m, k, with_c):
    """non-negative X, N, symmetric non-negative M1, M2; rows whose denominator falls under the 1e-10 floor; exact zeros"""
    X = rng.rand(m, k)
    N = rng.rand(m, k)
    B1, B2 = rng.rand(k + 3, k), rng.rand(k + 2, k)
    M1, M2 = B1.T @ B1, B2.T @ B2
    c = rng.rand(m) * 3. if with_c else None
    tiny = np.arange(m) % 7 == 3
    X[tiny] *= 1e-13                                   # X M + shift X ~ 1e-13 k: under the floor
    if with_c:
        c[tiny] *= 1e-3
    X[rng.rand(m, k) < 0.05] = 0.                      # exact zeros stay exact zeros
    if m > 2:
        X[2] = 0.
    return X, N, M1, M2, c


def check_update(got, X, N, M, a, lamb, c):
    """every entry within 1e-13 of the sum of the absolute values of the denominator's terms, carried through the division
    by the clamped denominator: |x a n / den^2| * 1e-13 * (|X| |M| + |shift| |x|)"""
    shift = lamb if c is None else (lamb + c)[:, None]
    den = np.maximum(X @ M + shift * X, ref.FLOOR)
    want = X * ((a * N) / den)
    terms = np.abs(X) @ np.abs(M) + np.abs(shift) * np.abs(X)
    bound = np.abs(want) / den * 1e-13 * terms
    err = np.abs(got - want)
    worst = float((err / np.where(bound > 0, bound, 1.))[bound > 0].max()) if (bound > 0).any() else 0.
    print('update %s: worst error / bound %.3g, clamped entries %d, zeros %d' % (X.shape, worst, int((den == ref.FLOOR).sum()),
                                                                               int((X == 0).sum())))
    assert (err <= bound).all()
    assert (got[X == 0] == 0).all()
    return den


@pytest.mark.parametrize('with_c', [False, True])
@pytest.mark.parametrize('rank', [1, 10, 16, 33, 50, 64, 100, 128, 130, 200])
@pytest.mark.parametrize('m', [1, 31, 32, 33, 1000, 100003])
def test_update_matches_numpy(hip_ops, m, rank, with_c):
    """the fused launch up to the bound (ranks 1..128: every column width of the kernel), the composition above it
    (130, 200); X and N with leading dimensions of their own; M = ma M1 + mb M2"""
    ops = hip_ops
    bound_rank = ops.lce_fused_max_rank()
    assert bound_rank == ref.FUSED_MAX_RANK == 128
    rng = np.random.RandomState(7 * rank + m + int(with_c))
    X, N, M1, M2, c = update_case(rng, m, rank, with_c)
    a, lamb, ma, mb = 0.37, 1e-12 if m % 2 else 0.8, 0.1, 0.9
    Xd, Nd = strided(ops, X), strided(ops, N, pad=5, off=2)
    cd = ops.to_device(c) if with_c else None
    from polara_amd import scoring
    rec = scoring._CallRecorder(ops.lib)
    ops.lib = rec
    try:
        out = ops.lce_update(Xd, Nd, ops.to_device(M1), ma=ma, M2=ops.to_device(M2), mb=mb, a=a, lamb=lamb, c=cd)
    finally:
        ops.lib = rec.lib
    rec_names = launches(rec)
    if rank <= bound_rank:
        assert rec_names == ['pk_lce_update_f64']
    else:
        assert rec_names == ['pk_axpbypcz_f64', 'pk_tsmm_f64', 'pk_lce_update_ew_f64']
    assert out is Xd
    den = check_update(ops.to_host(Xd), X, N, ma * M1 + mb * M2, a, lamb, c)
    if m >= 31:
        assert (den == ref.FLOOR).any()                  # the floor was met
    assert padding_is_zero(Xd)


@pytest.mark.parametrize('rank', [10, 50, 128])
def test_update_forms_agree(hip_ops, rank):
    """the fused launch and the composition on the same input, one M only: both within the bound of NumPy"""
    ops = hip_ops
    rng = np.random.RandomState(rank)
    X, N, M1, _, c = update_case(rng, 5000, rank, True)
    for fused in (True, False):
        Xd = ops.to_device(X)
        ops.lce_update(Xd, ops.to_device(N), ops.to_device(M1), ma=0.9, a=0.9, lamb=1.0, c=ops.to_device(c), fused=fused)
        check_update(ops.to_host(Xd), X, N, 0.9 * M1, 0.9, 1.0, c)
    with pytest.raises(Exception, match='rank'):
        big = ops.to_device(rng.rand(8, 130))
        ops.lce_update(big, big.clone(), ops.to_device(np.eye(130)), fused=True)


@pytest.mark.parametrize('m', [1, 33, 1000, 100003])
def test_reductions_match_numpy_in_a_fixed_order(hip_ops, m):
    ops = hip_ops
    rng = np.random.RandomState(m)
    k = 50
    P, Q, R = rng.randn(m, k), rng.randn(m, k), rng.randn(m, 7)
    w = rng.rand(m)
    G = rng.randn(k, k)
    Pd, Qd, Rd, wd, Gd = strided(ops, P), ops.to_device(Q), strided(ops, R, pad=1, off=0), ops.to_device(w), ops.to_device(G)
    pairs = [(-2.0, Pd, Qd, None), (0.5, Pd, Pd, wd), (1.0, Rd, None, None), (3.0, Gd.diagonal().unsqueeze(1), None, None),
             (0.25, Gd, Gd.t().contiguous(), None)]
    want = [np.sum(P * Q), np.sum(w[:, None] * P * P), np.sum(R), np.trace(G), np.sum(G * G.T)]
    mags = [np.sum(np.abs(P * Q)), np.sum(w[:, None] * P * P), np.sum(np.abs(R)), np.sum(np.abs(np.diag(G))), np.sum(np.abs(G * G.T))]
    out = ops.to_host(ops.lce_dots(pairs, bias=7.5))
    for p in range(len(pairs)):
        assert abs(out[1 + p] - want[p]) <= 1e-13 * mags[p], p
    obj = 7.5 + sum(c * v for (c, _, _, _), v in zip(pairs, out[1:]))
    assert abs(out[0] - obj) <= 1e-14 * (7.5 + sum(abs(c * v) for (c, _, _, _), v in zip(pairs, out[1:])))
    again = ops.to_host(ops.lce_dots(pairs, bias=7.5))
    assert np.array_equal(out.view(np.int64), again.view(np.int64))         # the same bits
    with pytest.raises(Exception):
        ops.lce_dots([(1.0, Pd, None, None)] * 17)


def test_clamp(hip_ops):
    ops = hip_ops
    rng = np.random.RandomState(1)
    for m, k in ((1, 1), (33, 7), (1000, 50)):
        E = rng.randn(m, k)
        Ed = strided(ops, E)
        assert ops.clamp_min(Ed, 0.0) is Ed
        assert np.array_equal(ops.to_host(Ed), np.maximum(E, 0.)) and padding_is_zero(Ed)


# ---- the solver ----------------------------------------------------------------------------------------------------------
def device_solve(ops, g, **over):
    from polara_amd import lce
    Xs, Xu, A, init, kw = ref.inputs(g)
    kw.update(over)
    stats = {}
    W, HuT, HsT = lce.local_collective_embeddings(ops, Xs, Xu, A, int(g['rank']), init=init, stats=stats, **kw)
    return W, HuT, HsT, stats


@pytest.mark.parametrize('name', FIXTURES)
def test_solver_matches_the_reference_fixtures(hip_ops, name):
    """factors within 1e-9 of the largest entry, objective history within 1e-9 relative, the same pass count; two builds of
    the same input: the same bits"""
    g = load_golden(name)
    ops = hip_ops
    W, HuT, HsT, stats = device_solve(ops, g)
    for got, want, what in ((W, g['W'], 'W'), (HuT, g['Hu'].T, 'Hu'), (HsT, g['Hs'].T, 'Hs')):
        err = np.abs(ops.to_host(got) - want).max() / np.abs(want).max()
        print('%s %s: error / largest entry %.3g' % (name, what, err))
        assert got.is_cuda and err <= TOL
    rel = np.abs(np.array(stats['objective']) / g['objective'] - 1.).max()
    print('%s objective: %d passes, relative error %.3g' % (name, stats['passes'], rel))
    assert stats['passes'] == len(g['objective']) and rel <= 1e-9
    W2, HuT2, HsT2, stats2 = device_solve(ops, g)
    assert torch.equal(W, W2) and torch.equal(HuT, HuT2) and torch.equal(HsT, HsT2)
    assert np.array_equal(np.array(stats['objective']).view(np.int64), np.array(stats2['objective']).view(np.int64))


def test_solver_composed_form_and_the_seeded_draw(hip_ops):
    g = load_golden('lce_std')
    ops = hip_ops
    W, HuT, HsT, stats = device_solve(ops, g, fused=False)
    assert close(ops.to_host(W), g['W']) and close(ops.to_host(HuT), g['Hu'].T) and close(ops.to_host(HsT), g['Hs'].T)
    assert stats['passes'] == len(g['objective'])
    # without init=: the reference's draw from the seed
    from polara_amd import lce
    Xs, Xu, A, _, kw = ref.inputs(g)
    W3, _, _ = lce.local_collective_embeddings(ops, Xs, Xu, A, int(g['rank']), seed=int(g['seed']), **kw)
    assert close(ops.to_host(W3), g['W'])


def test_library_calls_of_a_pass(hip_ops):
    """what DESIGN 8d reports: the library calls of one pass of the solver, recorded"""
    from polara_amd import scoring
    g = load_golden('lce_std')
    ops = hip_ops
    counts = []
    for maxiter in (1, 2):
        rec = scoring._CallRecorder(ops.lib)
        ops.lib = rec
        try:
            device_solve(ops, g, maxiter=maxiter, epsilon=0.0)
        finally:
            ops.lib = rec.lib
        counts.append(launches(rec))
    per_pass = counts[1][len(counts[0]):]
    print('library calls per pass:', len(per_pass), sorted((n, per_pass.count(n)) for n in set(per_pass)))
    assert len(counts[1]) - len(counts[0]) == len(per_pass)
    assert per_pass.count('pk_lce_update_f64') == 3 and per_pass.count('pk_lce_dots_f64') == 1
    assert per_pass.count('pk_spmm_csr_ex') == 5 and per_pass.count('pk_gram_f64') == 3
    assert set(per_pass) == {'pk_lce_update_f64', 'pk_lce_dots_f64', 'pk_spmm_csr_ex', 'pk_gram_f64'} and len(per_pass) == 12


# ---- recommend(queries=) -------------------------------------------------------------------------------------------------
def heavy_tailed_nonneg(rng, n, K):
    V = np.abs(rng.randn(n, K)) * np.exp(rng.randn(n, 1)) / np.sqrt(K)
    return np.ascontiguousarray(V[np.argsort(-np.linalg.norm(V, axis=1), kind='stable')])


def brute_seen(scores, seen, topk):
    """the lists under (unseen first, score desc, item asc): a partition of the unseen scores where a row has at least
    topk unseen items, the full three-key sort (i2i_reference.select) for the rows that have fewer"""
    from test_gpu_coldstart import brute_lists
    out = brute_lists(np.where(seen, -np.inf, scores), topk)
    few = np.flatnonzero((~seen).sum(axis=1) < topk)
    if len(few):
        out[few] = select(scores[few], seen[few], topk, True, False)
    return out, few


def count_tie_rows(lists, brute, scores, cls, tol):
    bad = tie_aware_mismatches(lists, brute, scores, cls, tol=tol)
    differ = np.flatnonzero((lists != brute).any(axis=1))
    return len(bad), len(set(differ.tolist()) - set(bad))


@pytest.mark.parametrize('n_users', [2005, 8205])
def test_recommend_with_queries_against_brute_force(hip_ops, n_users):
    """~40 000 items of non-negative factors with heavy-tailed norms, given user rows, seen items filtered; users with fewer
    than k unseen items; pruned and full sweeps identical; no row beyond ties, tie rows at most 1 in 1 000 (a bound the brute
    force in two summation orders keeps too).  8 205 users: the pass reorders the users by activity and the rows with them."""
    from polara_amd import scoring
    rng = np.random.RandomState(n_users)
    n_items, rank, topk = 40003, 50, 10
    V = heavy_tailed_nonneg(rng, n_items, rank)
    Q = heavy_tailed_nonneg(rng, n_users, rank)[rng.permutation(n_users)]
    rows, cols = [], []
    for u in range(n_users):
        if u in (3, 40, 1999):
            seen = np.setdiff1d(np.arange(n_items), rng.choice(n_items, topk - 1 - (u % 3), replace=False))   # fewer than k unseen
        else:
            seen = np.unique(rng.choice(n_items, rng.randint(1, 200 if u % 50 else 3000)))
        rows.append(np.full(len(seen), u))
        cols.append(seen)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    T = sps.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_users, n_items))
    seen_mask = np.zeros((n_users, n_items), dtype=bool)
    seen_mask[rows, cols] = True
    scores = Q @ V.T
    cls = np.where(seen_mask, 1, 2).astype(np.int8)              # i2i_reference.classes(dense): seen below unseen
    brute, few = brute_seen(scores, seen_mask, topk)
    assert len(few) == 3
    brute_rev, _ = brute_seen(Q[:, ::-1] @ V[:, ::-1].T, seen_mask, topk)          # the same sums in another order
    bad0, ties0 = count_tie_rows(brute_rev, brute, scores, cls, TIE_TOL)
    print('%d users, brute force in two orders: %d rows beyond ties, %d tie rows' % (n_users, bad0, ties0))
    assert bad0 == 0 and ties0 <= n_users // 1000
    ops = hip_ops
    image = scoring.FactorImage(ops, ops.to_device(V))
    Td = ops.csr(T.indptr, T.indices, T.data, T.shape)
    Qd = strided(ops, Q, pad=2, off=0)
    stats = {}
    pruned, s = scoring.recommend(ops, image, Td, topk, queries=Qd, return_scores=True, stats=stats)
    full = scoring.recommend(ops, image, Td, topk, queries=Qd, prune=False)
    ids = scoring.recommend(ops, image, Td, topk, queries=Qd)
    plain = scoring.recommend(ops, image, Td, topk, queries=Qd, order_users=False)
    got = ops.to_host(pruned)
    assert np.array_equal(got, ops.to_host(full)) and np.array_equal(got, ops.to_host(ids)) and np.array_equal(got, ops.to_host(plain))
    bad, ties = count_tie_rows(got, brute, scores, cls, TIE_TOL)
    print('%d users, device: %d rows beyond ties, %d tie rows, %d flagged, approximate fold-in %s' % (
        n_users, bad, ties, stats['flagged_users'], stats['approx_fold_in']))
    assert bad == 0 and ties <= n_users // 1000
    assert stats['approx_fold_in'] is False and stats['refolded_users'] == 0 and stats['flagged_users'] >= 3
    want = np.take_along_axis(scores, got, axis=1)
    assert np.abs(ops.to_host(s) - want).max() <= 1e-12 * np.abs(scores).max()
    # the default is untouched: without queries the pass folds in
    assert np.array_equal(ops.to_host(scoring.recommend(ops, image, Td, topk)), ops.to_host(scoring.recommend(ops, image, Td, topk, queries=None)))


# ---- the models ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_models_match_the_reference_fixtures(hip_ops, name):
    g = load_golden(name)
    check_lce_model_against_fixture(ref.model_for(g, hip_ops), g)


def test_cold_start_keeps_the_user_factors_and_maps_ids_on_the_device(hip_ops):
    from polara_amd import scoring
    g = load_golden('lce_cs_rank7')
    ops = hip_ops
    m = ref.model_for(g, ops)
    m.build()
    kept = m._factors_dev
    assert kept is not None and kept[0] is m.factors['userid'] and kept[1].is_cuda and kept[2].is_cuda
    assert isinstance(m.factors['userid'], np.ndarray)
    image, order = m._user_factors_device()
    assert np.array_equal(ops.to_host(image.V), m.factors['userid'][order])
    E = m._cold_queries_device()
    assert ops.sweep_takes_rows(E) and E.stride(0) % 2 == 0 and float(E.min()) >= 0.0
    rec = scoring._CallRecorder(ops.lib)
    ops.lib = rec
    try:
        again = m.get_recommendations()
    finally:
        ops.lib = rec.lib
    names = launches(rec)
    assert np.array_equal(again, g['recs'])
    assert 'pk_spmm_csr_ex' in names and 'pk_tsmm_f64' in names and 'pk_clamp_min_f64' in names and 'pk_map_ids_i64' in names
    swept = sweeps(rec.calls)
    assert swept and all(s['E'] and not s['Ep'] and not s['user_bound'] for s in swept), swept       # from rows, not packed
    assert 'pk_pack_frag_bound_f32' not in names and 'pk_row_norm_order_f64' not in names     # the image is the build's


# ---- at scale --------------------------------------------------------------------------------------------------------------
def test_planted_case_at_scale(hip_ops):
    """~20 000 items x 100 000 users, 3 000 labels, rank 50 against the restatement: the tolerances of the fixtures, lists
    compared tie-aware, no row beyond ties"""
    from polara_amd import lce, scoring
    rng = np.random.RandomState(2024)
    n_items, n_users, n_labels, k, topk = 20011, 100003, 3000, 50, 10
    zi, zu = rng.randint(0, 40, n_items), rng.randint(0, 40, n_users)
    per = rng.randint(8, 60, n_users)
    urows = np.repeat(np.arange(n_users), per)
    # a user draws mostly from its own cluster of items
    own = rng.rand(len(urows)) < 0.7
    by_cluster = [np.flatnonzero(zi == c) for c in range(40)]
    ucols = rng.randint(0, n_items, len(urows))
    pick = rng.rand(len(urows))
    for c in range(40):
        sel = np.flatnonzero(own & (zu[urows] == c))
        ucols[sel] = by_cluster[c][(pick[sel] * len(by_cluster[c])).astype(np.int64)]
    XuT = sps.csr_matrix((rng.randint(1, 6, len(urows)).astype(np.float64), (urows, ucols)), shape=(n_users, n_items))
    XuT.sum_duplicates()
    Xu = XuT.T.tocsr()
    lrows = np.repeat(np.arange(n_items), 4)
    lcols = (zi[lrows] * 75 + rng.randint(0, 75, len(lrows))) % n_labels
    Xs = sps.csr_matrix((np.ones(len(lrows)), (lrows, lcols)), shape=(n_items, n_labels))
    Xs.sum_duplicates()
    Xs.data[:] = 1.
    nb = np.concatenate([np.arange(n_items)[:, None], rng.randint(0, n_items, (n_items, 10))], axis=1)
    A = sps.csr_matrix((np.ones(nb.size), (np.repeat(np.arange(n_items), 11), nb.ravel())), shape=(n_items, n_items))
    A.sum_duplicates()
    A.data[:] = 1.
    init = lce.initial_factors(n_items, n_labels, n_users, k, seed=5)
    kw = dict(alpha=0.1, beta=0.05, lamb=1., epsilon=1e-4, maxiter=15)
    Wr, HuTr, HsTr, hist = ref.solve(Xs, Xu, A, *init, **kw)
    deltas = np.abs(np.diff(hist))
    assert np.maximum(deltas / kw['epsilon'], kw['epsilon'] / deltas).min() >= 1.01          # the stopping rule is not on an edge
    ops = hip_ops
    stats = {}
    W, HuT, HsT = lce.local_collective_embeddings(ops, Xs, Xu, A, k, init=init, stats=stats, **kw)
    for got, want, what in ((W, Wr, 'W'), (HuT, HuTr, 'Hu'), (HsT, HsTr, 'Hs')):
        err = np.abs(ops.to_host(got) - want).max() / np.abs(want).max()
        print('scale %s: error / largest entry %.3g' % (what, err))
        assert err <= TOL
    rel = np.abs(np.array(stats['objective']) / np.array(hist) - 1.).max()
    print('scale objective: %d passes, relative error %.3g' % (stats['passes'], rel))
    assert stats['passes'] == len(hist) and rel <= 1e-9
    # the standard pass for the first 3 000 users against brute force on the restatement's factors
    n_test = 3000
    order_dev, _, Ws = ops.norm_order(W)
    order = ops.to_host(order_dev).astype(np.int64)             # the catalogue order of the pass (any order serves the brute force)
    rank_of = np.empty(n_items, dtype=np.int64)
    rank_of[order] = np.arange(n_items)
    T = XuT[:n_test].tocoo()
    Ti = sps.csr_matrix((T.data, (T.row, rank_of[T.col])), shape=(n_test, n_items))
    Ti.sort_indices()
    seen = np.zeros((n_test, n_items), dtype=bool)
    seen[T.row, rank_of[T.col]] = True
    scores = HuTr[:n_test] @ Wr[order].T
    cls = np.where(seen, 1, 2).astype(np.int8)
    brute, _ = brute_seen(scores, seen, topk)
    Qd = strided(ops, ops.to_host(HuT[:n_test]), pad=0, off=0)
    got = ops.to_host(scoring.recommend(ops, scoring.FactorImage(ops, Ws), ops.csr(Ti.indptr, Ti.indices, Ti.data, Ti.shape), topk,
                                        queries=Qd))
    bad, ties = count_tie_rows(got, brute, scores, cls, TIE_TOL)
    print('scale lists: %d rows beyond ties, %d tie rows of %d' % (bad, ties, n_test))
    assert bad == 0
