"""Item cold start on the device: the query operator (`HipOps.coldstart_queries`) against NumPy, `scoring.recommend_dense` against
brute-force fp64, and every model against the reference's fixtures (tests/golden/coldstart_*.npz)."""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

import coldstart_reference as ref
from conftest import load_golden
from i2i_reference import tie_aware_mismatches
from recorded_calls import sweeps
from test_coldstart_host import FACTOR_FIXTURES, check_model_against_fixture, model_for

pytestmark = pytest.mark.gpu


def random_features(rng, n_cold, n_labels, weighted, empty_every=5):
    rows = []
    for c in range(n_cold):
        k = 0 if (empty_every and c % empty_every == 2) else int(rng.randint(1, min(n_labels, 9) + 1))
        rows.append(np.sort(rng.choice(n_labels, k, replace=False)))
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
    indices = (np.concatenate(rows) if len(rows) else np.zeros(0)).astype(np.int32)
    values = rng.rand(len(indices)) + 0.5 if weighted else None
    return indptr, indices, values


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('rank', [1, 10, 50, 64, 100, 130, 256, 300])
@pytest.mark.parametrize('n_cold', [1, 31, 32, 33, 1000])
def test_query_operator_matches_numpy(hip_ops, n_cold, rank, weighted):
    """fp64 sums in another order than NumPy's: every entry within 1e-13 of the sum of the absolute values of its terms
    ((nnz of a row + rank) roundings of 1.1e-16 each, at most ~310 of them here: 3.4e-14), padding columns zero, rows without
    features exactly zero; W with a leading dimension of its own."""
    rng = np.random.RandomState(1000 * rank + n_cold + int(weighted))
    n_labels = 37
    indptr, indices, values = random_features(rng, n_cold, n_labels, weighted, empty_every=0 if n_cold == 1 else 5)
    Wfull = rng.randn(n_labels, rank + 3)
    G = rng.randn(rank, rank)
    G = G + G.T
    ops = hip_ops
    Wd = ops.to_device(Wfull)[:, 1:1 + rank]                     # strided view: ldw = rank + 3
    assert Wd.stride(0) == rank + 3
    Fd = ops.csr(indptr, indices, np.ones(len(indices)) if values is None else values, (n_cold, n_labels))
    E = ops.coldstart_queries(Fd, Wd, ops.to_device(G))
    assert tuple(E.shape) == (n_cold, rank) and E.stride(0) % 2 == 0 and E.stride(0) >= rank and E.data_ptr() % 16 == 0
    assert ops.sweep_takes_rows(E)
    block = torch.as_strided(E, (n_cold, E.stride(0)), (E.stride(0), 1))
    got, pad = ops.to_host(E), ops.to_host(block)[:, rank:]
    W = Wfull[:, 1:1 + rank]
    want = ref.queries(indptr, indices, values, W, G)
    F = sps.csr_matrix((np.ones(len(indices)) if values is None else values, indices, indptr), shape=(n_cold, n_labels))
    bound = 1e-13 * (np.asarray(F @ np.abs(W)) @ np.abs(G))
    assert (np.abs(got - want) <= bound).all()
    assert (pad == 0).all()
    empty = np.diff(indptr) == 0
    assert (got[empty] == 0).all()


def heavy_tailed(rng, n, K):
    V = rng.randn(n, K) * np.exp(rng.randn(n, 1)) / np.sqrt(K)
    return np.ascontiguousarray(V[np.argsort(-np.linalg.norm(V, axis=1), kind='stable')])


def brute_lists(scores, topk):
    part = np.argpartition(-scores, topk, axis=1)[:, :topk + 1] if scores.shape[1] > topk + 1 else np.tile(np.arange(scores.shape[1]), (scores.shape[0], 1))
    out = np.empty((scores.shape[0], topk), dtype=np.int64)
    for r in range(scores.shape[0]):
        cand = part[r]
        # everything tied with the k-th score must be in the pool for the index tie-break to be the total order's
        kth = np.sort(scores[r, cand])[::-1][topk - 1]
        cand = np.union1d(cand, np.flatnonzero(scores[r] == kth))
        out[r] = cand[np.lexsort((cand, -scores[r, cand]))][:topk]
    return out


def count_tie_rows(lists, brute, scores, tol):
    """(rows that fail the tie-aware check, rows that differ from the brute-force list and yet pass it)"""
    cls = np.broadcast_to(np.ones(1, dtype=np.int64), scores.shape)
    bad = tie_aware_mismatches(lists, brute, scores, cls, tol=tol)
    differ = np.flatnonzero((lists != brute).any(axis=1))
    return len(bad), len(set(differ.tolist()) - set(bad))


# scores here are O(1) sums of <= 100 fp64 products: two summation orders differ by at most ~100 * 1.1e-16 * sum |terms|,
# far below 1e-12 — the tolerance at which two scores count as tied
TIE_TOL = 1e-12


@pytest.mark.parametrize('rank', [50, 100])
def test_recommend_dense_against_brute_force(hip_ops, rank):
    """~40 000 catalogue rows x ~2 000 queries of continuous random factors, heavy-tailed row norms; top-10 and top-20, pruned
    and full sweeps give identical lists; no row fails the tie-aware comparison with the brute-force fp64 lists, and rows that
    differ from them yet pass it (ties at the accuracy of fp64) are at most 1 in 1 000 — a bound the brute force itself,
    summed in two different orders on the CPU, must keep too."""
    from polara_amd import scoring
    rng = np.random.RandomState(rank)
    n_cat, n_q = 40003, 2005
    V = heavy_tailed(rng, n_cat, rank)
    Eh = rng.randn(n_q, rank)
    Eh[5] = 0                                         # an empty query: zero scores, any k rows are a valid answer
    scores = Eh @ V.T
    scores_rev = Eh[:, ::-1] @ V[:, ::-1].T            # the same sums in another order
    ops = hip_ops
    image = scoring.FactorImage(ops, ops.to_device(V))
    block = torch.zeros(n_q, rank + (rank & 1), dtype=torch.float64, device=ops.device)
    block[:, :rank] = ops.to_device(Eh)
    E = block[:, :rank]
    for topk in (10, 20):
        brute = brute_lists(scores, topk)
        bad0, ties0 = count_tie_rows(brute_lists(scores_rev, topk), brute, scores, TIE_TOL)
        print('rank %d top-%d brute force, two orders: %d rows beyond ties, %d tie rows' % (rank, topk, bad0, ties0))
        assert bad0 == 0 and ties0 <= n_q // 1000
        stats = {}
        pruned, s = scoring.recommend_dense(ops, image, E, topk, return_scores=True, stats=stats)
        full = scoring.recommend_dense(ops, image, E, topk, prune=False)
        pruned_ids = scoring.recommend_dense(ops, image, E, topk)
        got = ops.to_host(pruned)
        assert np.array_equal(got, ops.to_host(full)) and np.array_equal(got, ops.to_host(pruned_ids))
        bad, ties = count_tie_rows(got, brute, scores, TIE_TOL)
        print('rank %d top-%d device: %d rows beyond ties, %d tie rows, %d flagged, tiles %d of %d' % (
            rank, topk, bad, ties, stats['flagged_users'], stats['tiles_scored'], stats['tiles_total']))
        assert bad == 0 and ties <= n_q // 1000
        sh = ops.to_host(s)
        want = np.take_along_axis(scores, got, axis=1)
        assert np.abs(sh - want).max() <= 1e-12 * np.abs(scores).max()
        assert stats['tiles_scored'] < stats['tiles_total']          # the pruning bound bites on heavy-tailed norms


@pytest.mark.parametrize('n_q,n_cat,rank,topk', [(40, 3001, 50, 60), (7, 5000, 50, 10), (31, 2000, 10, 10), (10, 2000, 300, 10)])
def test_recommend_dense_small_and_exact_routes(hip_ops, n_q, n_cat, rank, topk):
    """top-k beyond the fused capacity (52) and a rank beyond 256 take the exact-row route; fewer than 32 queries are one
    partial group of the sweep; a strided query block without the sweep's alignment goes through the packing launch"""
    from polara_amd import scoring
    rng = np.random.RandomState(n_q + rank + topk)
    V = heavy_tailed(rng, n_cat, rank)
    Eh = rng.randn(n_q, rank)
    scores = Eh @ V.T
    ops = hip_ops
    image = scoring.FactorImage(ops, ops.to_device(V))
    brute = brute_lists(scores, topk)
    got = ops.to_host(scoring.recommend_dense(ops, image, ops.to_device(Eh), topk))
    assert count_tie_rows(got, brute, scores, TIE_TOL) == (0, 0)
    odd = torch.zeros(n_q, rank + 3, dtype=torch.float64, device=ops.device)     # odd leading dimension / offset start
    odd[:, 1:1 + rank] = ops.to_device(Eh)
    got2 = ops.to_host(scoring.recommend_dense(ops, image, odd[:, 1:1 + rank], topk))
    assert np.array_equal(got, got2)
    out = torch.empty(n_q, topk, dtype=torch.int64, device=ops.device)
    assert scoring.recommend_dense(ops, image, ops.to_device(Eh), topk, out=out) is out and np.array_equal(ops.to_host(out), got)
    with pytest.raises(ValueError):
        scoring.recommend_dense(ops, image, ops.to_device(Eh), n_cat + 1)


@pytest.mark.parametrize('name', FACTOR_FIXTURES)
def test_models_match_the_reference_fixtures(hip_ops, name):
    """sigma to rtol 1e-9, W / projectors / factors up to column signs to 1e-8, scores to 1e-9 relative, lists and lists after
    rank = 5 equal, evaluate() equal to the stored numbers — the tolerances of tests/test_gpu_hybrid.py for the same factors"""
    g = load_golden(name)
    m = model_for(g, hip_ops)
    check_model_against_fixture(m, g)


def test_model_keeps_the_user_factors_on_the_device(hip_ops):
    g = load_golden('coldstart_svd')
    m = model_for(g, hip_ops)
    m.build()
    kept = m._user_factors_dev
    assert kept is not None and kept[0] is m.factors['userid'] and kept[1].is_cuda
    assert isinstance(m.factors['userid'], np.ndarray) and m.factors['userid'].shape == g['U'].shape
    image, order = m._user_factors_device()
    X = m.factors['userid'] * m.factors['singular_values'][None, :]
    assert np.allclose(hip_ops.to_host(image.V), X[order], rtol=1e-14, atol=0)
    # the pass reads the queries straight from the rows the query kernel wrote (no packing launch), maps the catalogue
    # positions to user ids on the device, and runs as the library calls listed here
    from polara_amd import scoring
    E = m._cold_queries_device()
    assert hip_ops.sweep_takes_rows(E) and E.stride(0) % 2 == 0 and E.data_ptr() % 16 == 0
    m.collect_recommend_stats = True
    m._recommendations = None
    recs = m.recommendations
    assert np.array_equal(recs, g['recs']) and m.recommend_stats['candidate_capacity'] == 16
    m.collect_recommend_stats = False
    rec = scoring._CallRecorder(hip_ops.lib)
    hip_ops.lib = rec
    try:
        again = m.get_recommendations()
    finally:
        hip_ops.lib = rec.lib
    names = [n for n, _, _ in rec.calls]
    assert np.array_equal(again, g['recs'])
    assert 'pk_spmm_csr_ex' in names and 'pk_tsmm_f64' in names and 'pk_map_ids_i64' in names
    swept = sweeps(rec.calls)
    assert swept and all(s['E'] and not s['Ep'] and not s['user_bound'] for s in swept), swept       # from rows, not packed
    assert 'pk_pack_frag_bound_f32' not in names
