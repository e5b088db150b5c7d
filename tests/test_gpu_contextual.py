"""Contextual post-filtering on the device (csrc/context.hip): pk_context_merge_f64 against the NumPy restatement of the
class order (tests/contextual_reference.py) at every place the kernel takes another path — empty lists, one window, several
rounds, the window edges, every class, seen and exhausted rows, pads — its scores against the bits of the base pass, and the
model layer (fixture from the reference itself; a model with explicit user factors; the plain path untouched)."""
import numpy as np
import pytest
import torch

import contextual_reference as cref
from conftest import load_golden

from polara_amd import _lib, scoring
from polara_amd.contextual import ItemPostFilteringMixin
from polara_amd.data import ItemPostFilteringArrayData
from polara_amd.models import SVDModel

pytestmark = pytest.mark.gpu

W = _lib.load().pk_context_window()


def padded(ops, a, pad):
    """device copy of the fp64 block `a` with `pad` extra columns in its leading dimension"""
    t = ops.zeros(a.shape[0], a.shape[1] + pad)
    t[:, :a.shape[1]] = ops.to_device(a)
    return t[:, :a.shape[1]]


def device_case(ops, V, E, sp, si, topk, filter_seen, pad_v=0, pad_e=0):
    """(image, T, E on the device, base lists of the plain pass from those query rows)"""
    image = scoring.FactorImage(ops, ops.to_device(V))
    T = ops.csr(sp, si, np.ones(len(si)), (E.shape[0], V.shape[0]))
    Ed = padded(ops, E, pad_e)
    base = scoring.recommend(ops, image, T, topk, filter_seen, queries=Ed)
    Vd = padded(ops, V, pad_v) if pad_v else image.V
    return Vd, T, Ed, base


def merge(ops, Vd, T, Ed, ctx, base, filter_seen, order=None, n_items=None):
    n_users, n_items = Ed.shape[0], Vd.shape[0]
    lists = [ops.context_lists(uv, ptr, items, n_users, n_items) for uv, ptr, items in ctx]
    seen = (T.indptr, T.indices) if filter_seen else None
    out, cls = ops.context_merge(Vd, Ed, seen, lists, base, want_class=True,
                                 order=None if order is None else ops.to_device(order.astype(np.int32)))
    torch.cuda.synchronize()
    return ops.to_host(out), ops.to_host(cls)


@pytest.mark.parametrize('filter_seen', [True, False])
def test_kernel_matches_the_numpy_class_order(hip_ops, filter_seen):
    ops = hip_ops
    V, E, sp, si, ctx = cref.construction(sizes_a=(0, 1, 3, 40, W + 404, 7))
    scores = E @ V.T
    seen = cref.seen_mask(sp, si, *scores.shape) if filter_seen else np.zeros(scores.shape, dtype=bool)
    gap = cref.min_gap(scores, seen, 10)
    tier_gap = cref.class_order_gap(scores, ctx, seen, 10)
    print('min gap of the reference scores over ranks 1..11: %.3g plain, %.3g in class order' % (gap, tier_gap))
    assert gap > 1e-6 and tier_gap > 1e-6
    want_ids, want_cls = cref.class_order_lists(scores, ctx, seen, 10)
    Vd, T, Ed, base = device_case(ops, V, E, sp, si, 10, filter_seen)
    assert np.array_equal(ops.to_host(base), cref.plain_lists(scores, seen, 10))
    by_value = np.argsort(ctx[0][0], kind='stable')
    for order in (None, by_value):
        ids, cls = merge(ops, Vd, T, Ed, ctx, base, filter_seen, order)
        assert np.array_equal(ids, want_ids) and np.array_equal(cls, want_cls)       # every row
    assert set(np.unique(want_cls)) == {0, 1, 2, 3}


def test_window_edges(hip_ops):
    ops = hip_ops
    topk, K, n_items = 10, 4, 2 * W + 50
    lengths = [topk - 1, topk, W - 1, W, W + 1, 2 * W - topk, 2 * W - topk + 1, n_items]
    rng = np.random.RandomState(6)
    V, E = rng.rand(n_items, K), rng.rand(len(lengths), K)
    lists = [np.sort(rng.choice(n_items, n, replace=False)) for n in lengths]
    ctx = [(np.arange(len(lengths), dtype=np.int32), np.r_[0, np.cumsum(lengths)].astype(np.int64), np.concatenate(lists).astype(np.int32))]
    si = np.concatenate([np.sort(rng.choice(n_items, 6, replace=False)) for _ in lengths]).astype(np.int32)
    sp = np.arange(len(lengths) + 1, dtype=np.int64) * 6
    scores = E @ V.T
    seen = cref.seen_mask(sp, si, *scores.shape)
    gap = cref.min_gap(scores, seen, topk)
    ctx2 = [(np.full(len(lengths), 7, dtype=np.int32), ctx[0][1], ctx[0][2]), ctx[0]]
    tier_gap = min(cref.class_order_gap(scores, c, seen, topk) for c in (ctx, ctx2))
    print('min gap: %.3g plain, %.3g in class order' % (gap, tier_gap))
    assert gap > 1e-6 and tier_gap > 1e-6
    want_ids, want_cls = cref.class_order_lists(scores, ctx, seen, topk)
    Vd, T, Ed, base = device_case(ops, V, E, sp, si, topk, True)
    ids, cls = merge(ops, Vd, T, Ed, ctx, base, True)
    assert np.array_equal(ids, want_ids) and np.array_equal(cls, want_cls)
    # a second context behind it: its rounds start with carried entries (window - topk new ones per round)
    want_ids, want_cls = cref.class_order_lists(scores, ctx2, seen, topk)
    ids, cls = merge(ops, Vd, T, Ed, ctx2, base, True)
    assert np.array_equal(ids, want_ids) and np.array_equal(cls, want_cls)


@pytest.mark.parametrize('K', [1, 5, 16, 50])
def test_same_bits_as_the_base_pass(hip_ops, K):
    """one context whose single value lists the whole catalogue: the tier IS the plain order, so any difference in the bits
    of a score would show as a swapped pair somewhere in 64 x 5 000 Gaussian scores"""
    ops = hip_ops
    n_users, n_items = 64, 5000
    rng = np.random.RandomState(K)
    V, E = rng.randn(n_items, K), rng.randn(n_users, K)
    V[1::7] = V[0::7][:len(V[1::7])]              # duplicated item rows: exact ties, resolved by ascending position
    si = np.concatenate([np.sort(rng.choice(n_items, 20, replace=False)) for _ in range(n_users)]).astype(np.int32)
    sp = np.arange(n_users + 1, dtype=np.int64) * 20
    ctx = [(np.zeros(n_users, dtype=np.int32), np.array([0, n_items], dtype=np.int64), np.arange(n_items, dtype=np.int32))]
    for topk in (1, 10, 52, 100):
        for filter_seen in (True, False):
            Vd, T, Ed, base = device_case(ops, V, E, sp, si, topk, filter_seen, pad_v=2 if K % 2 == 0 else 3, pad_e=6)
            ids, cls = merge(ops, Vd, T, Ed, ctx, base, filter_seen)
            base = ops.to_host(base)
            assert np.array_equal(ids, base), (K, topk, filter_seen)                  # every row, nothing excluded
            assert (cls == 1).all()
    pairs = [(a, b) for row in base for a, b in zip(row[:-1], row[1:]) if a % 7 == 0 and b == a + 1]
    assert len(pairs) > 0                          # tied pairs do occur in the lists, lower position first


def test_corners(hip_ops):
    ops = hip_ops
    n_items, K, topk = 40, 4, 10
    rng = np.random.RandomState(11)
    V, E = rng.rand(n_items, K), rng.rand(5, K)
    list_a, list_b = np.array([1, 4, 9, 12, 20, 33]), np.array([4, 5, 12, 30])
    ctx = [(np.array([0, 0, -1, 0, 0], dtype=np.int32), np.array([0, 6], dtype=np.int64), list_a.astype(np.int32)),
           (np.array([-1, 0, -1, 0, -1], dtype=np.int32), np.array([0, 4], dtype=np.int64), list_b.astype(np.int32))]
    seen_rows = [list_a,                                               # user 0: every context item seen
                 np.setdiff1d(np.arange(n_items), [4, 7, 20, 21, 30]),   # user 1: five unseen items, three of them context items
                 np.array([0, 3]),                                     # user 2: no value in any context
                 np.array([2, 9]),                                     # user 3: both contexts, overlapping: classes 3, 2, 1
                 np.array([], dtype=np.int64)]                         # user 4: nothing seen
    si = np.concatenate(seen_rows).astype(np.int32)
    sp = np.r_[0, np.cumsum([len(r) for r in seen_rows])].astype(np.int64)
    scores = E @ V.T
    seen = cref.seen_mask(sp, si, *scores.shape)
    Vd, T, Ed, base = device_case(ops, V, E, sp, si, topk, True)
    base_h = ops.to_host(base)
    assert np.array_equal(base_h, cref.plain_lists(scores, seen, topk))     # user 1's seen tail included
    ids, cls = merge(ops, Vd, T, Ed, ctx, base, True)
    want_ids, want_cls = cref.class_order_lists(scores, ctx, seen, topk)
    assert np.array_equal(ids, want_ids) and np.array_equal(cls, want_cls)
    assert np.array_equal(ids[0], base_h[0]) and (cls[0] == 0).all()
    assert np.array_equal(ids[2], base_h[2]) and (cls[2] == 0).all()
    assert ids[1][:3].tolist() == [4, 30, 20] and cls[1].tolist() == [3, 2, 1] + [0] * 7 and sorted(ids[1][3:5]) == [7, 21]
    assert np.array_equal(ids[1][5:], base_h[1][5:]) and seen[1, ids[1][5:]].all()       # the seen tail in base order
    assert cls[3].tolist() == [3, 3, 2, 2, 1, 1, 1, 0, 0, 0] and sorted(ids[3][:2]) == [4, 12] and sorted(ids[3][2:4]) == [5, 30]
    # pads carry through: a hand-made base whose rows end in -1 (what a catalogue shorter than topk would give)
    short = base_h.copy()
    short[:, 6:] = -1
    out, ocls = ops.context_merge(Vd, Ed, (T.indptr, T.indices), [ops.context_lists(*c, 5, n_items) for c in ctx],
                                  ops.to_device(short), want_class=True)
    want, wcls = cref.merge_reference(V, E, sp, si, ctx, short, scores=scores)
    assert np.array_equal(ops.to_host(out), want) and np.array_equal(ops.to_host(ocls), wcls)
    assert (want[2, 6:] == -1).all() and (want[0, 6:] == -1).all()
    # filter_seen off: the seen context items of user 0 come first
    Vd, T, Ed, base = device_case(ops, V, E, sp, si, topk, False)
    ids, cls = merge(ops, Vd, T, Ed, ctx, base, False)
    want_ids, want_cls = cref.class_order_lists(scores, ctx, np.zeros_like(seen), topk)
    assert np.array_equal(ids, want_ids) and np.array_equal(cls, want_cls) and sorted(ids[0][:6]) == list_a.tolist()


# ---- models ---------------------------------------------------------------------------------------------------------------
class ContextualSVD(ItemPostFilteringMixin, SVDModel):
    pass


def test_mixin_over_svd_equals_the_reference_lists(hip_ops):
    from test_contextual_host import fixture_data
    g = load_golden('contextual_small')
    m = ContextualSVD(fixture_data(g), ops=hip_ops)
    m.verbose = False
    m.rank, m.topk = int(g['rank']), int(g['topk'])
    m.collect_recommend_stats = True
    m.build()
    assert np.allclose(m.factors['singular_values'], g['singular_values'], rtol=1e-9)
    assert np.array_equal(m.get_recommendations(), g['recs'])
    assert (m.recommend_stats['context_class'] > 0).any()
    m.context_order_users = not m.context_order_users
    m._context_dev = None
    assert np.array_equal(m.get_recommendations(), g['recs'])
    plain = SVDModel(m.data, ops=hip_ops)
    plain.verbose = False
    plain.rank, plain.topk = m.rank, m.topk
    plain.build()
    assert np.array_equal(plain.get_recommendations(), g['plain_recs'])


def ials_data(seed=2, n_users=300, n_items=400):
    rng = np.random.RandomState(seed)
    rows = [np.sort(rng.choice(n_items, rng.randint(6, 30), replace=False)) for _ in range(n_users)]
    hold_items = np.array([r[rng.randint(len(r))] for r in rows])
    u = np.concatenate([np.full(len(r) - 1, k) for k, r in enumerate(rows)])
    i = np.concatenate([r[r != h] for r, h in zip(rows, hold_items)])
    genre = rng.randint(0, 8, n_items)
    tag_items = rng.choice(n_items, 150, replace=False)
    mapping = {'genre': (np.arange(n_items), genre), 'tag': (tag_items, rng.randint(0, 3, len(tag_items)))}
    test_users = np.sort(rng.choice(n_users, 120, replace=False))
    holdout = (test_users, hold_items[test_users], np.ones(len(test_users)))
    hc = {'genre': genre[hold_items[test_users]], 'tag': rng.randint(0, 4, len(test_users))}
    return ItemPostFilteringArrayData((u, i, rng.randint(1, 6, len(u)).astype(np.float64)), n_users=n_users, n_items=n_items, holdout=holdout, warm_start=False,
                                      item_context_mapping=mapping, holdout_context=hc)


def test_mixin_over_explicit_user_factors_and_the_plain_path(hip_ops):
    from polara_amd.ials import ImplicitALS

    class ContextualALS(ItemPostFilteringMixin, ImplicitALS):
        pass
    data = ials_data()
    m = ContextualALS(data, ops=hip_ops, seed=3)
    m.verbose = False
    m.rank, m.topk, m.num_epochs = 16, 10, 4
    m.build()
    recs = m.get_recommendations()
    test_data, shape, test_users = m._get_test_data()
    P, Q = m.factors[data.fields.userid], m.factors[data.fields.itemid]
    scores = P[test_users] @ Q.T
    seen = np.zeros(scores.shape, dtype=bool)
    seen[test_data[0], test_data[1]] = True
    ctx = [(data.user_context(c),) + tuple(data.context_values(c)[1:]) for c in data.contexts]
    gap, tier_gap = cref.min_gap(scores, seen, 10), cref.class_order_gap(scores, ctx, seen, 10)
    print('min gap: %.3g plain, %.3g in class order' % (gap, tier_gap))
    assert gap > 1e-9 and tier_gap > 1e-9          # far above the rounding of a 16-term fp64 dot product of O(1) scores
    want, _ = cref.class_order_lists(scores, ctx, seen, 10)
    assert np.array_equal(recs, want) and (recs != cref.plain_lists(scores, seen, 10)).any()
    # the same model without the mixin: exactly what scoring.recommend gives when called directly
    plain = ImplicitALS(data, ops=hip_ops, seed=3)
    plain.verbose = False
    plain.rank, plain.topk, plain.num_epochs = 16, 10, 4
    plain.build()
    assert np.array_equal(plain.factors[data.fields.itemid], Q)
    T, n_users, _ = plain._device_test_csr()
    direct = scoring.recommend(hip_ops, plain._item_factors_device(), T, 10, True, queries=plain._test_queries(test_users))
    assert np.array_equal(plain.get_recommendations(), plain._external_ids(direct, plain._item_inv))
    assert np.array_equal(plain.get_recommendations(), cref.plain_lists(scores, seen, 10))
