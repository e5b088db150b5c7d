"""Sampled-negatives evaluation on the device (csrc/sampled.hip): pk_candidates_topk_f64 and pk_sample_unseen against the
NumPy restatements of tests/sampled_reference.py — scores bit-equal, lists and sampled ids equal — and the models against the
fixtures the reference itself produced (tests/golden/make_golden_sampled.py).

Tolerances: the kernel against the restatement, fed the same P, V and candidates: none (the sums run in the same order with
separately rounded multiplies and adds).  The models against the reference: rtol 1e-9, atol 1e-10 on the scores — what
tests/test_gpu_models.py holds dense score rows to (the device builds its own V) — and equal lists on EVERY row: the fixtures
were generated with a gap of more than 1e-6 * max|score| between consecutive top-(k+1) scores of every row."""
import numpy as np
import pytest

import sampled_reference as ref
from conftest import load_golden
from test_sampled_host import FIXTURES, fixture_data

pytestmark = pytest.mark.gpu


def candidate_case(n_users, n_items, r, C, seed):
    rng = np.random.RandomState(seed)
    P = rng.randn(n_users, r)
    V = rng.randn(n_items, r)
    cand = rng.randint(0, n_items, (n_users, C))
    cand[0, 0], cand[-1, -1] = 0, n_items - 1          # the ends of the catalogue
    if C > 1:
        cand[:, 1] = cand[:, 0]                         # a repeated candidate in every row: equal scores, the lower position first
    return P, V, cand.astype(np.int32)


def run_candidates(ops, P, V, cand, topk, want_scores=True, column_major=False):
    Pd, Vd = ops.to_device(P), ops.to_device(V)
    if column_major:
        Vd = Vd.t().contiguous().t()
        assert Vd.stride(0) == 1 or Vd.shape[1] == 1
    lists, scores = ops.candidates_topk(Pd, Vd, ops.to_device(cand), topk, want_scores=want_scores)
    return ops.to_host(lists), (None if scores is None else ops.to_host(scores))


@pytest.mark.parametrize('r', [1, 7, 50, 100])
def test_candidates_against_the_restatement(hip_ops, r):
    n_items = 301
    for n_users in (1, 70):
        for C in (6, 64, 65, 1000, 1025):
            P, V, cand = candidate_case(n_users, n_items, r, C, seed=1000 * r + C + n_users)
            want_scores = ref.gathered_scores(P, V, cand)
            for topk in (1, 10, C):
                if topk > C:
                    continue
                want = ref.select(want_scores, topk)
                lists, scores = run_candidates(hip_ops, P, V, cand, topk)
                assert lists.dtype == np.int64 and lists.shape == (n_users, topk)
                assert np.array_equal(scores.view(np.int64), want_scores.view(np.int64)), (n_users, C, topk)      # bit-equal
                assert np.array_equal(lists, want), (n_users, C, topk)
            quiet, none = run_candidates(hip_ops, P, V, cand, min(10, C), want_scores=False)
            assert none is None and np.array_equal(quiet, ref.select(want_scores, min(10, C)))


def test_candidates_layouts_and_repeats(hip_ops):
    """A column-major V (the layout of the host factors), an odd rank (the 16-byte path ends in a single element; an odd
    leading dimension takes the 8-byte path), a P with a leading dimension, two calls with identical bytes."""
    P, V, cand = candidate_case(33, 97, 9, 130, seed=5)
    want_scores = ref.gathered_scores(P, V, cand)
    want = ref.select(want_scores, 130)
    for column_major in (False, True):
        lists, scores = run_candidates(hip_ops, P, V, cand, 130, column_major=column_major)
        assert np.array_equal(scores.view(np.int64), want_scores.view(np.int64)) and np.array_equal(lists, want)
    # every row repeats its first candidate at position 1: the tie resolves to the lower position
    pos0, pos1 = (want == 0).argmax(axis=1), (want == 1).argmax(axis=1)
    assert (pos1 == pos0 + 1).all()
    ops = hip_ops
    wide = ops.to_device(np.concatenate((P, np.full((33, 3), 7.0)), axis=1))[:, :9]       # leading dimension 12
    even = ops.to_device(np.concatenate((V, np.full((97, 1), 7.0)), axis=1))[:, :9]       # leading dimension 10: 16-byte loads
    a = ops.candidates_topk(wide, even, ops.to_device(cand), 10, want_scores=True)
    b = ops.candidates_topk(wide, even, ops.to_device(cand), 10, want_scores=True)
    for x, y in zip(a, b):
        assert ops.to_host(x).tobytes() == ops.to_host(y).tobytes()
    assert np.array_equal(ops.to_host(a[1]).view(np.int64), want_scores.view(np.int64))
    assert np.array_equal(ops.to_host(a[0]), want[:, :10])


def test_candidates_above_the_fused_limit(hip_ops):
    limit = hip_ops.lib.pk_candidates_fused_max()
    assert limit >= 4096
    for C, topk in ((limit, 10), (limit + 5, 10), (limit + 5, limit + 5)):
        P, V, cand = candidate_case(3, 211, 7, C, seed=C + topk)
        want_scores = ref.gathered_scores(P, V, cand)
        for want_s in (True, False):
            lists, scores = run_candidates(hip_ops, P, V, cand, topk, want_scores=want_s)
            assert np.array_equal(lists, ref.select(want_scores, topk)), (C, topk)
            assert scores is None or np.array_equal(scores.view(np.int64), want_scores.view(np.int64))


def test_candidates_bad_arguments(hip_ops):
    from polara_amd._lib import PolaraHipError
    ops = hip_ops
    P, V, cand = candidate_case(4, 50, 5, 8, seed=1)
    with pytest.raises(PolaraHipError):
        run_candidates(ops, P, V, cand, 9)                       # topk > C
    with pytest.raises(PolaraHipError):
        run_candidates(ops, P, V, cand, 0)
    big = ops.lib.pk_candidates_max_rank() + 1
    with pytest.raises(PolaraHipError):
        run_candidates(ops, np.zeros((4, big)), np.zeros((50, big)), cand, 3)
    # the ids are validated on the host, before any launch
    for bad in (-1, 50):
        c = cand.copy()
        c[2, 3] = bad
        with pytest.raises(ValueError):
            run_candidates(ops, P, V, c, 3)
    with pytest.raises(ValueError):
        run_candidates(ops, P, V[:, :4], cand, 3)
    lib = ops.lib
    assert lib.pk_candidates_topk_f64(None, 4, 50, 5, None, 5, None, 5, 1, None, 8, 3, None, None) != 0     # null pointers


# ---- the sampler -----------------------------------------------------------------------------------------------------------
def sample_both(ops, rows, hold, n_items, n, seed=0):
    t_ptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
    t_idx = (np.concatenate(rows) if len(t_ptr) > 1 and t_ptr[-1] else np.zeros(0)).astype(np.int32)
    seeds = np.random.SeedSequence(seed).generate_state(len(rows))
    T = ops.csr(t_ptr, t_idx, np.ones(len(t_idx)), (len(rows), n_items))
    if hold is None:
        H, h_ptr, h_idx = None, None, None
    else:
        h_ptr = np.r_[0, np.cumsum([len(r) for r in hold])].astype(np.int64)
        h_idx = np.concatenate([np.asarray(r, dtype=np.int32) for r in hold]).astype(np.int32)
        H = ops.csr(h_ptr, h_idx, np.ones(len(h_idx)), (len(rows), n_items))
    got = ops.to_host(ops.sample_unseen(T, H, n, seeds))
    return got, ref.sample_unseen(t_ptr, t_idx, h_ptr, h_idx, n_items, n, seeds)


def test_sampler_against_the_restatement(hip_ops):
    rng = np.random.RandomState(3)
    n_items, n = 97, 12                                         # not a power of two: the mapping rejects draws
    rows = [np.zeros(0, dtype=np.int64),                        # an empty row
            np.sort(rng.choice(n_items, 85, replace=False)),    # exactly n eligible items, a row longer than 64 entries
            np.array([0, 96]),                                  # the ends of the catalogue excluded
            np.sort(rng.choice(n_items, 30, replace=False))]
    hold = [[5], [], [1, 95], [int(rows[3][0])]]                # (the last one also sits in the row: the union counts)
    got, want = sample_both(hip_ops, rows, hold, n_items, n, seed=11)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert sorted(got[1].tolist()) == sorted(set(range(n_items)) - set(rows[1].tolist()))
    got, want = sample_both(hip_ops, rows, None, n_items, n, seed=11)         # no second exclusion
    assert np.array_equal(got, want)
    got, want = sample_both(hip_ops, rows, hold, n_items, 1, seed=12)         # n = 1
    assert got.shape == (4, 1) and np.array_equal(got, want)
    # more users than one wave per compute unit can hide, a power-of-two catalogue, n beyond one round of 64 draws
    rows = [np.sort(rng.choice(512, rng.randint(0, 200), replace=False)) for _ in range(300)]
    hold = [rng.choice(512, 2, replace=False).tolist() for _ in range(300)]
    got, want = sample_both(hip_ops, rows, hold, 512, 150, seed=13)
    assert np.array_equal(got, want)
    for u in range(300):
        assert len(set(got[u].tolist())) == 150 and not set(got[u].tolist()) & (set(rows[u].tolist()) | set(hold[u]))


def test_sampler_refuses_on_the_host(hip_ops):
    rows = [np.arange(0, 90), np.zeros(0, dtype=np.int64)]
    with pytest.raises(ValueError, match='fewer than'):
        sample_both(hip_ops, rows, [[95], [3]], 97, 7)                          # user 0 has 97 - 91 = 6 eligible items
    got, want = sample_both(hip_ops, rows, [[95], [3]], 97, 6, seed=1)          # exactly enough
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        sample_both(hip_ops, rows, None, 97, 98, seed=1)
    T = hip_ops.csr(np.array([0, 1]), np.array([1], dtype=np.int32), np.ones(1), (1, 50))
    with pytest.raises(ValueError):
        hip_ops.sample_unseen(T, None, 5, np.arange(2))                         # a seed per user
    # a launch whose round limit would exceed what one wave may take is refused, on the host and by the library
    lib = hip_ops.lib
    n_items = 1 << 20
    assert lib.pk_sample_round_limit(n_items, 100, 100) > lib.pk_sample_max_rounds() > lib.pk_sample_round_limit(n_items, 100, n_items // 2)
    tight = hip_ops.csr(np.array([0, n_items - 100]), np.arange(n_items - 100, dtype=np.int32), np.ones(n_items - 100), (1, n_items))
    with pytest.raises(ValueError, match='rounds'):
        hip_ops.sample_unseen(tight, None, 100, np.arange(1))
    assert lib.pk_sample_unseen(None, 1, n_items, 1, None, None, None, 100, 100, 1, 1, 1) != 0     # refused before any pointer is read


# ---- the models on the reference's fixtures ------------------------------------------------------------------------------
def built_model(hip_ops, g, cls=None, **kw):
    from polara_amd import SVDModelSampled
    m = (cls or SVDModelSampled)(fixture_data(g, **kw), ops=hip_ops)
    m.verbose = False
    m.rank, m.topk = int(g['rank']), int(g['topk'])
    m.build()
    return m


@pytest.mark.parametrize('name', FIXTURES)
def test_models_on_the_fixtures(hip_ops, name):
    g = load_golden(name)
    m = built_model(hip_ops, g)
    lists, scores, items = m.recommend_with_scores()
    h = int(g['holdout_size'])
    assert np.array_equal(items, np.concatenate((g['hold_item'].reshape(-1, h), g['unseen']), axis=1))
    err = np.abs(scores - g['scores'])
    print('%s: max |score error| %.3e (max |score| %.3e)' % (name, err.max(), np.abs(g['scores']).max()))
    assert np.allclose(scores, g['scores'], rtol=1e-9, atol=1e-10)
    assert np.array_equal(lists, g['recs'])                                     # every row
    assert np.array_equal(m.get_recommendations(), g['recs']) and m.recommendations is m.recommendations
    for kind in ('relevance', 'ranking', 'hits'):
        got = m.evaluate(kind)
        assert [str(x) for x in g['metric_%s_names' % kind]] == list(got._fields)
        for field, w in zip(got._fields, g['metric_%s' % kind]):
            v = getattr(got, field)
            assert (v is None or np.isnan(v)) if np.isnan(w) else v == pytest.approx(w, rel=1e-12, abs=0), (kind, field)
    # the three score functions: host arrays in, host arrays out, bit-equal to the reference's for its own factors
    hs = m.compute_holdout_scores(g['user_factors'], np.asfortranarray(g['V']))
    us = m.compute_random_item_scores(g['user_factors'], np.asfortranarray(g['V']))
    assert np.array_equal(np.concatenate((hs, us), axis=1), g['scores'])


def test_rank_truncation(hip_ops):
    """`m.rank = 5` after a rank-10 build: the lists are the restatement's for the truncated factors on EVERY row.  The
    restatement is fed the device's own fold-in P (as in test_sampled_path), so the scores are bit-equal; against a fold-in
    recomputed on the host they agree to the tolerance of the fixture test."""
    from scipy.sparse import csr_matrix
    g = load_golden('sampled_h3')
    m = built_model(hip_ops, g)
    full = m.get_recommendations()
    m.rank = 5
    lists, scores, items = m.recommend_with_scores()
    V5 = m.factors['itemid']
    assert V5.shape[1] == 5
    P, Vd, cand = m.sampled_candidates()
    assert tuple(P.shape) == (lists.shape[0], 5) and tuple(Vd.shape) == (V5.shape[0], 5)
    want_lists, want_scores = ref.candidates_topk(hip_ops.to_host(P), V5, items, int(g['topk']))
    assert np.array_equal(scores.view(np.int64), want_scores.view(np.int64))
    assert np.array_equal(lists, want_lists)                                    # every row
    T = csr_matrix((g['test_fdbk'], (g['test_user'], g['test_item'])), shape=tuple(int(x) for x in g['test_shape']))
    assert np.allclose(scores, ref.gathered_scores(T.dot(V5), V5, items), rtol=1e-9, atol=1e-10)
    assert np.array_equal(m.get_recommendations(), lists) and not np.array_equal(lists, full)


def test_scaled_model_runs_the_protocol(hip_ops):
    from polara_amd import ScaledSVDSampled
    g = load_golden('sampled_h1')
    m = built_model(hip_ops, g, cls=ScaledSVDSampled)
    lists, scores, _ = m.recommend_with_scores()
    assert np.array_equal(lists, ref.select(scores, int(g['topk']))) and m.method != 'ABC'


@pytest.mark.parametrize('name', ['sampled_h1', 'sampled_h3'])
def test_sampled_path(hip_ops, name):
    g = load_golden(name)
    n_unseen, h = 29, int(g['holdout_size'])
    m = built_model(hip_ops, g, with_unseen=False, seed=3)
    with pytest.raises(ValueError, match='Number of items to sample is unspecified.'):
        m.get_recommendations()
    m.data.unseen_items_num = n_unseen
    lists, scores, items = m.recommend_with_scores()
    n_users, n_items = (int(x) for x in g['test_shape'])
    # the ids are the sampler's for the data's seed, over the data's item ids whatever order the model keeps internally
    t_ptr = np.r_[0, np.cumsum(np.bincount(g['test_user'], minlength=n_users))]
    order = np.lexsort((g['test_item'], g['test_user']))
    hold = g['hold_item'].reshape(-1, h)
    h_ptr = np.arange(n_users + 1) * h
    seeds = np.random.SeedSequence(3).generate_state(n_users)
    want_unseen = ref.sample_unseen(t_ptr, g['test_item'][order], h_ptr, hold.ravel(), n_items, n_unseen, seeds)
    assert np.array_equal(items[:, :h], hold) and np.array_equal(items[:, h:], want_unseen)
    for u in range(n_users):
        seen = set(g['test_item'][g['test_user'] == u].tolist()) | set(hold[u].tolist())
        assert not seen & set(items[u, h:].tolist())
    # the lists are candidates_topk applied to those ids
    assert np.array_equal(lists, ref.select(scores, int(g['topk'])))
    assert np.array_equal(m.get_recommendations(), lists)
    V = m.factors['itemid']
    P, Vd, cand = m.sampled_candidates()
    again, _ = hip_ops.candidates_topk(P, Vd, cand, int(g['topk']))
    assert np.array_equal(hip_ops.to_host(again), lists)
    want_scores = ref.gathered_scores(hip_ops.to_host(P), V, items)
    assert np.array_equal(scores, want_scores)                                  # the same P: bit-equal
    hr = m.evaluate('relevance')
    assert 0.0 <= hr[0] <= 1.0
